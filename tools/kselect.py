"""What the keypoint selection (nm_sift_select_batch_dev) costs beside a copy of the bytes it moves, and what it buys the
blind matcher, on the GPU.

    python tools/kselect.py [--pairs 16] [--rounds 20] [--keep 2048] [--trace]

Input: 2 x `pairs` of the bench's synthetic 1080p frames (uniform noise, Gaussian pre-blur; about 12k keypoints each),
detected once. Arms, each bracketed by device events on one stream and alternated round by round after warm-up:
    select     the four select launches for 64 frames (the detected frames, repeated to fill 64 slots; every slot has its
               own outputs): default score, 16 x 9 grid, x / y / desc / kpts / orients gathered, out_index written;
    copy       device-to-device copies of the bytes that call reads and writes: every frame's m descriptor rows read once
               (512 B a row, copied: read and written) stands for the score pass, and `keep` rows of x, y, desc, kpts,
               orients for the gather;
    full       nm_sift_match_batch_dev_f32 on `pairs` pairs at full size (about 12k x 12k);
    selected   select to `keep` rows on both frames of every pair, then the same matcher on the selected sets.
Frame 0's device selection is checked against the host twin first. Prints one JSON line with medians and min-max,
select / copy and full / selected. Not measured here: RANSAC and refit on full, selected and first-`keep` sets.
--trace runs only a few calls of each arm (for a kernel trace in a run of its own).
"""
import argparse

import numpy as np

import karms
import torch

import niftymatch_amd as nm
from niftymatch_amd import synth

W, H, CAP = 1920, 1080, 16384
GX, GY = 16, 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--keep", type=int, default=2048)
    karms.timing_args(ap, rounds=20, warmup=3, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kselect.py measures on a GPU"
    assert 1 <= a.pairs <= 32
    dev = torch.device("cuda:0")
    n, keep = a.pairs, a.keep
    taps, r = nm.create_kernel_for_sigma(synth.preblur_sigma(W, H))
    taps_d = torch.from_numpy(taps).to(dev)
    frames = [nm.convolve(synth.noise_frame_torch(s, W, H, dev), taps_d, r) for s in range(2 * n)]
    arenas = [nm.SiftArena(W, H, CAP, device=dev) for _ in range(2 * n)]
    for c in range(0, 2 * n, 16):
        nm.detect_describe_batch(arenas[c:c + 16], frames[c:c + 16])
    torch.cuda.synchronize()
    del frames
    rows = [int(x.num_items.item()) for x in arenas]
    stream = torch.cuda.Stream()

    slots = [arenas[k % (2 * n)] for k in range(64)]
    col = lambda name, src: [getattr(x, name) for x in src]
    ws64 = nm.SelectWorkspace(64, CAP, GX, GY, dev)
    held = {}

    def select64():
        held["s64"] = nm.sift_select_batch_dev(col("num_items", slots), col("x", slots), col("y", slots), W, H,
                                               descs=col("desc", slots), kpts=col("kpts", slots), orients=col("orients", slots),
                                               gx=GX, gy=GY, keep=keep, capacity=CAP, out=held.get("s64"), workspace=ws64)

    spare_desc = [torch.zeros((CAP, 128), dtype=torch.float32, device=dev) for _ in range(64)]
    spare_small = [torch.zeros((CAP, 8), dtype=torch.float32, device=dev) for _ in range(64)]

    def copy64():                                        # 512 B a row read + written, then keep rows of 512 + 32 B
        for k, x in enumerate(slots):
            m = rows[k % (2 * n)]
            spare_desc[k][:m].copy_(x.desc[:m])
            spare_desc[k][:keep].copy_(x.desc[:keep])
            spare_small[k][:keep, :4].copy_(x.kpts[:keep])
            spare_small[k][:keep, 4:6].copy_(x.orients[:keep])
            spare_small[k][:keep, 6].copy_(x.x[:keep])
            spare_small[k][:keep, 7].copy_(x.y[:keep])

    nA, nB = col("num_items", arenas[0::2]), col("num_items", arenas[1::2])
    full_res = [torch.full((CAP,), -1, dtype=torch.int32, device=dev) for _ in range(n)]
    sel_res = [torch.full((keep,), -1, dtype=torch.int32, device=dev) for _ in range(n)]
    mws = nm.MatchBatchDevWorkspace(n, CAP, CAP, dev)
    sws = nm.MatchBatchDevWorkspace(n, keep, keep, dev)
    ws_pairs = nm.SelectWorkspace(2 * n, CAP, GX, GY, dev)

    def full():
        nm.sift_match_batch_dev(col("desc", arenas[0::2]), nA, col("desc", arenas[1::2]), nB, full_res, 0.8, workspace=mws,
                                capA=CAP, capB=CAP)

    def selected():
        s = nm.sift_select_batch_dev(col("num_items", arenas), col("x", arenas), col("y", arenas), W, H, descs=col("desc", arenas),
                                     gx=GX, gy=GY, keep=keep, capacity=CAP, out=held.get("sp"), workspace=ws_pairs)
        held["sp"] = s
        cnt = [s["count"][k:k + 1] for k in range(2 * n)]
        nm.sift_match_batch_dev(s["desc"][0::2], cnt[0::2], s["desc"][1::2], cnt[1::2], sel_res, 0.8, workspace=sws, capA=keep,
                                capB=keep)

    arms = {"select_64_frames": select64, "copy_same_bytes": copy64, "full_match": full, "select_and_match": selected}
    with torch.cuda.stream(stream):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    if a.trace:
        with torch.cuda.stream(stream):
            for _ in range(5):
                for fn in arms.values():
                    fn()
        torch.cuda.synchronize()
        karms.emit({"tool": "kselect", "trace_calls": 5, "pairs": n})
        return

    x0 = arenas[0]
    cpu = lambda t: t.cpu().numpy()
    host = nm.sift_select_host([rows[0]], [cpu(x0.x)], [cpu(x0.y)], W, H, descs=[cpu(x0.desc)], gx=GX, gy=GY, keep=keep, capacity=CAP)
    c0 = int(host["count"][0])
    assert int(held["s64"]["count"][0]) == c0 and np.array_equal(cpu(held["s64"]["index"][0])[:c0], host["index"][0][:c0]), \
        "device and host twin differ (frame 0)"
    assert np.array_equal(cpu(held["s64"]["desc"][0])[:c0].view(np.uint32), host["desc"][0][:c0].view(np.uint32))

    sp = karms.spread(karms.time_eager(arms, stream, a.rounds, a.warmup))
    med = sp["median_us"]
    moved = sum(rows[k % (2 * n)] * 512 + min(keep, rows[k % (2 * n)]) * 2 * (512 + 32 + 4) for k in range(64))
    karms.emit({"tool": "kselect", "pairs": n, "rounds": a.rounds, "keep": keep, "grid": [GX, GY], "rows": rows[:4], **sp,
                "select_over_copy": med["select_64_frames"] / med["copy_same_bytes"],
                "select_us_per_frame": med["select_64_frames"] / 64, "select_bytes_per_s": moved / (med["select_64_frames"] * 1e-6),
                "full_over_selected": med["full_match"] / med["select_and_match"],
                "matches_pair0": {"full": int((full_res[0] >= 0).sum()), "selected": int((sel_res[0] >= 0).sum())}})
    for x in arenas:
        x.close()


if __name__ == "__main__":
    main()
