"""What the u8 k-nearest-neighbour entry (nm_sift_match_knn_u8_batch_dev) costs beside the u8 matcher on the same
descriptors, on the GPU.

    python tools/kknn_u8.py [--pairs 16] [--rounds 20] [--rows N] [--trace] [--out FILE]

Input: `pairs` frame pairs of the bench's synthetic 1080p frames (uniform noise, Gaussian pre-blur; about 12k keypoints
each), detected once, finished once (NM_DESC_L2, u8). Arms, each bracketed by device events on one stream and alternated
round by round after warm-up:
    match   nm_sift_match_u8_batch_dev on the bytes: the yardstick;
    knn1, knn2, knn4, knn8   nm_sift_match_knn_u8_batch_dev at k = 1, 2, 4, 8, indices and distances.
Pair 0 of every arm is checked against its host twin first, and the k = 2 lists of every pair, put through the matcher's
last step, against the matcher's result. Prints one JSON line (and writes it to --out): medians with min-max, per pair, and
each k's ratio to the matcher. --rows N clips every frame's row count to N. --trace runs only a few calls of each arm (for
a kernel trace in a run of its own; the arms are match_scan_u8_kernel<2, RatioOut> and <L, ListOut>, L = 1, 2, 4, 8).
"""
import argparse
import json

import numpy as np

import karms
import torch

import niftymatch_amd as nm
from niftymatch_amd import synth

W, H, CAP = 1920, 1080, 16384
KS = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--rows", type=int, default=0, help="use at most this many rows of every frame (0: all)")
    ap.add_argument("--out", default=None, help="a file of its own for the record, indented (written anew)")
    karms.timing_args(ap, rounds=20, warmup=3, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kknn_u8.py measures on a GPU"
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
    counts = [x.num_items for x in arenas]
    if a.rows:
        counts = [torch.clamp(c, max=a.rows) for c in counts]
    u8 = [torch.zeros((CAP, 128), dtype=torch.uint8, device=dev) for _ in range(2 * n)]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        nm.desc_finish_batch_dev([x.desc for x in arenas], counts, out_u8=u8, capacity=CAP)
    torch.cuda.synchronize()
    A, B, nA, nB = u8[0::2], u8[1::2], counts[0::2], counts[1::2]
    res = [torch.full((CAP,), -1, dtype=torch.int32, device=dev) for _ in range(n)]
    idx = {k: [torch.full((CAP, k), -1, dtype=torch.int32, device=dev) for _ in range(n)] for k in KS}
    dist = {k: [torch.full((CAP, k), 0x7fffffff, dtype=torch.int32, device=dev) for _ in range(n)] for k in KS}
    uws = nm.MatchU8Workspace(n, CAP, CAP, dev)
    kws = nm.MatchKnnU8Workspace(n, CAP, CAP, dev)

    def match():
        nm.sift_match_u8_batch_dev(A, nA, B, nB, results=res, ambiguity=0.8, workspace=uws, capA=CAP, capB=CAP)

    def knn(k):
        return lambda: nm.sift_match_knn_u8_batch_dev(A, nA, B, nB, k, indices=idx[k], distances=dist[k], workspace=kws,
                                                      capA=CAP, capB=CAP)

    arms = {"match": match}
    arms.update({"knn%d" % k: knn(k) for k in KS})
    if a.trace:
        with torch.cuda.stream(stream):
            for _ in range(5):
                for fn in arms.values():
                    fn()
        torch.cuda.synchronize()
        karms.emit({"tool": "kknn_u8", "trace_calls": 5, "pairs": n})
        return

    with torch.cuda.stream(stream):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    rows = [int(x.item()) for x in counts]
    a0, b0 = A[0].cpu().numpy(), B[0].cpu().numpy()
    host = nm.sift_match_u8_host([a0], [rows[0]], [b0], [rows[1]], ambiguity=0.8, capA=CAP, capB=CAP, prior=-1)
    assert np.array_equal(res[0].cpu().numpy(), host[0]), "matcher: device and host twin differ (pair 0)"
    for k in KS:
        hi, hd = nm.sift_match_knn_u8_host([a0], [rows[0]], [b0], [rows[1]], k, capA=CAP, capB=CAP)
        assert np.array_equal(idx[k][0].cpu().numpy(), hi[0]), "k-NN index: device and host twin differ (pair 0, k %d)" % k
        assert np.array_equal(dist[k][0].cpu().numpy(), hd[0]), "k-NN distance: device and host twin differ (pair 0, k %d)" % k
    for p in range(n):                                   # the matcher's last step on the k = 2 lists (nB > 1 here)
        i2, d2 = idx[2][p][:rows[2 * p]], dist[2][p][:rows[2 * p]].float()
        want = torch.where(d2[:, 0] / d2[:, 1] < 0.8, i2[:, 0], torch.full_like(i2[:, 0], -1))
        want = torch.where(d2[:, 1] > 0, want, res[p][:rows[2 * p]])
        assert torch.equal(want, res[p][:rows[2 * p]]), "k = 2 lists and the matcher differ (pair %d)" % p

    sp = karms.spread(karms.time_eager(arms, stream, a.rounds, a.warmup))
    med = sp["median_us"]
    out = {"tool": "kknn_u8", "pairs": n, "rounds": a.rounds, "rows": rows[:4], **sp,
           "us_per_pair": {k: v / n for k, v in med.items()},
           "over_matcher": {k: v / med["match"] for k, v in med.items() if k != "match"}}
    karms.emit(out)
    if a.out:                                            # not emit's appended line: profiles/ keeps this record indented
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    for x in arenas:
        x.close()


if __name__ == "__main__":
    main()
