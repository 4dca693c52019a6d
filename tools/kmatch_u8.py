"""What the u8 matcher (nm_sift_match_u8_batch_dev) costs beside the fp32 matcher on the same descriptors, and what the
descriptor finish costs beside a copy of the same bytes, on the GPU.

    python tools/kmatch_u8.py [--pairs 16] [--rounds 20] [--rows N] [--trace]

Input: `pairs` frame pairs of the bench's synthetic 1080p frames (uniform noise, Gaussian pre-blur; about 12k keypoints
each), detected once, finished once (NM_DESC_L2; fp32 and u8 outputs). Arms, each bracketed by device events on one stream
and alternated round by round after warm-up:
    a  nm_sift_match_batch_dev_f32 on the float copies of the u8 rows: the yardstick, what a client runs today;
    b  nm_sift_match_u8_batch_dev on the bytes;
    finish  the finish launch of all 2 x pairs frames (fp32 in, fp32 + u8 out);
    copy    device-to-device copies of every frame's fp32 and u8 rows (1280 B moved per row; the finish moves 1152 B).
Pair 0's device result is checked against the host twin first, and arm (b)'s results against arm (a)'s for every pair.
Prints one JSON line: medians with min-max, b / a, arm (b)'s share of the i8 matrix peak, the finish's bytes per second.
--rows N clips every frame's row count to N (--pairs 1 --rows 4096: one small pair, where a scan is a few tiles).
--trace runs only a few calls of each arm (for a kernel trace in a run of its own; arm (b) is match_u8_norms_kernel and
match_scan_u8_kernel<2, RatioOut>).
"""
import argparse

import numpy as np

import karms
import torch

import niftymatch_amd as nm
from niftymatch_amd import synth

W, H, CAP = 1920, 1080, 16384
I8_PEAK_OPS = 5.0e15                           # twice the ~2.5 PF dense bf16 peak: the same cycles per MFMA at twice the K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--rows", type=int, default=0, help="use at most this many rows of every frame (0: all)")
    karms.timing_args(ap, rounds=20, warmup=3, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kmatch_u8.py measures on a GPU"
    assert 1 <= a.pairs <= nm.MATCH_MAX_BATCH
    dev = torch.device("cuda:0")
    n = a.pairs
    taps, r = nm.create_kernel_for_sigma(synth.preblur_sigma(W, H))
    taps_d = torch.from_numpy(taps).to(dev)
    frames = [nm.convolve(synth.noise_frame_torch(s, W, H, dev), taps_d, r) for s in range(2 * n)]
    arenas = [nm.SiftArena(W, H, CAP, device=dev) for _ in range(2 * n)]
    for c in range(0, 2 * n, 16):
        nm.detect_describe_batch(arenas[c:c + 16], frames[c:c + 16])
    torch.cuda.synchronize()
    del frames
    descs, counts = [x.desc for x in arenas], [x.num_items for x in arenas]
    if a.rows:
        counts = [torch.clamp(c, max=a.rows) for c in counts]
    f32 = [torch.zeros((CAP, 128), dtype=torch.float32, device=dev) for _ in range(2 * n)]
    u8 = [torch.zeros((CAP, 128), dtype=torch.uint8, device=dev) for _ in range(2 * n)]
    stream = torch.cuda.Stream()

    def finish():
        nm.desc_finish_batch_dev(descs, counts, out_f32=f32, out_u8=u8, capacity=CAP)

    with torch.cuda.stream(stream):
        finish()
    torch.cuda.synchronize()
    flt = [u.float() for u in u8]
    nA, nB = counts[0::2], counts[1::2]
    full = lambda: [torch.full((CAP,), -1, dtype=torch.int32, device=dev) for _ in range(n)]
    ra, rb = full(), full()
    mws = nm.MatchBatchDevWorkspace(n, CAP, CAP, dev)
    uws = nm.MatchU8Workspace(n, CAP, CAP, dev)

    def arm_a():
        nm.sift_match_batch_dev(flt[0::2], nA, flt[1::2], nB, ra, 0.8, workspace=mws, capA=CAP, capB=CAP)

    def arm_b():
        nm.sift_match_u8_batch_dev(u8[0::2], nA, u8[1::2], nB, results=rb, ambiguity=0.8, workspace=uws, capA=CAP, capB=CAP)

    if a.trace:
        with torch.cuda.stream(stream):
            for _ in range(5):
                arm_a()
                arm_b()
                finish()
        torch.cuda.synchronize()
        karms.emit({"tool": "kmatch_u8", "trace_calls": 5, "pairs": n})
        return

    with torch.cuda.stream(stream):
        arm_a()
        arm_b()
    torch.cuda.synchronize()
    rows = [int(x.item()) for x in counts]
    host = nm.sift_match_u8_host([u8[0].cpu().numpy()], [rows[0]], [u8[1].cpu().numpy()], [rows[1]], ambiguity=0.8, capA=CAP,
                                 capB=CAP, prior=-1)
    assert np.array_equal(rb[0].cpu().numpy(), host[0]), "device and host twin differ (pair 0)"
    for k in range(n):
        assert torch.equal(ra[k], rb[k]), "u8 matcher and fp32 matcher on float copies differ (pair %d)" % k
    hf, hu = nm.desc_finish_host([descs[0].cpu().numpy()], [rows[0]], capacity=CAP)
    assert np.array_equal(u8[0].cpu().numpy()[:rows[0]], hu[0][:rows[0]]), "finish: device and host twin differ (u8)"
    assert np.array_equal(f32[0].cpu().numpy()[:rows[0]].view(np.uint32), hf[0][:rows[0]].view(np.uint32)), "finish (f32)"

    spare = [torch.zeros((CAP, 128), dtype=torch.uint8, device=dev) for _ in range(2 * n)]

    def copy():                                          # 1280 B per row (fp32 and u8 rows, read and written) against 1152
        for d, f, u, s, c in zip(descs, f32, u8, spare, rows):
            f[:c].copy_(d[:c])
            s[:c].copy_(u[:c])

    arms = {"a_f32_matcher_on_float_copies": arm_a, "b_u8_matcher": arm_b, "finish": finish, "copy_same_bytes": copy}
    sp = karms.spread(karms.time_eager(arms, stream, a.rounds, a.warmup))
    med = sp["median_us"]
    ops = sum(2.0 * 128 * rows[2 * k] * rows[2 * k + 1] for k in range(n))
    moved = sum(rows) * (512 + 640)
    karms.emit({"tool": "kmatch_u8", "pairs": n, "rounds": a.rounds, "rows": rows[:4], "matches_pair0": int((rb[0] >= 0).sum()), **sp,
                "b_over_a": med["b_u8_matcher"] / med["a_f32_matcher_on_float_copies"],
                "b_us_per_pair": med["b_u8_matcher"] / n,
                "b_share_of_i8_peak": ops / (med["b_u8_matcher"] * 1e-6) / I8_PEAK_OPS,
                "finish_bytes_per_s": moved / (med["finish"] * 1e-6), "finish_over_copy": med["finish"] / med["copy_same_bytes"]})
    for x in arenas:
        x.close()


if __name__ == "__main__":
    main()
