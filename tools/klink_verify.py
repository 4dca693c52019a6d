"""What the link verification (nm_link_verify_batch_dev_f32) costs beside the refit call it follows, on the GPU.

    python tools/klink_verify.py [--pairs 16] [--rounds 20] [--trace]

16 pairs of 1920 x 1080 gray planes (17 frames, frame k + 1 is B of pair k and A of pair k + 1; each is the one before
shifted by a few pixels, so the maps are true) at strides 1, 2 and 4, and tools/kransac_refit.py's refit call, each
bracketed by device events on one stream; rounds alternate the four after warm-up. The device outputs are checked against
the host twin before timing. Prints one JSON line: medians with min-max, and per stride the bytes the call must move
(A's lattice values, 4 bytes each, plus B's gathered lines: every 64-byte line of B that holds a tap, which at strides
1 to 4 is all of B) so that the time can be set against tools/hbm_probe.py's bandwidth. --trace runs only a few calls
(for `rocprofv3 --kernel-trace --stats`: launches per call, kernel times; no counters).
"""
import argparse

import numpy as np

import karms
import torch

import niftymatch_amd as nm

from kransac_refit import noisy_pair

FW, FH = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    karms.timing_args(ap, rounds=20, warmup=3, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "klink_verify.py measures on a GPU"
    dev = torch.device("cuda:0")
    n = a.pairs
    rng = np.random.default_rng(0)
    base = (255 * rng.random((FH + 64, FW + 4 * n + 64), dtype=np.float32)).astype(np.float32)
    frames = [np.ascontiguousarray(base[3 * (k % 2):3 * (k % 2) + FH, 4 * k:4 * k + FW]) for k in range(n + 1)]
    H = np.stack([np.array([1, 0, -4, 0, 1, 3 * (k % 2) - 3 * ((k + 1) % 2), 0, 0, 1], np.float32) for k in range(n)])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_frames, d_H = [t(f) for f in frames], t(H)
    ws = nm.LinkVerifyWorkspace(n, dev)
    stream = torch.cuda.Stream()
    strides = (1, 2, 4)

    def verify(s):
        return nm.link_verify_batch_dev(d_frames[:-1], d_frames[1:], d_H, stride=s, workspace=ws)

    if a.trace:
        with torch.cuda.stream(stream):
            for _ in range(5):
                for s in strides:
                    verify(s)
        torch.cuda.synchronize()
        karms.emit({"tool": "klink_verify", "trace_calls": 5 * len(strides), "pairs": n})
        return

    stats = {}
    for s in strides:
        with torch.cuda.stream(stream):
            out = verify(s)
        torch.cuda.synchronize()
        host = nm.link_verify_host(frames[:-1], frames[1:], H, stride=s)
        for d, h in zip(out, host):
            assert np.array_equal(d.cpu().numpy().view(np.uint8), h.view(np.uint8)), "device and host twin differ"
        stats[s] = {"ncc_min": float(host[2][:, 3].min()), "overlap_min": float(host[2][:, 2].min()),
                    "passed": int(host[0].sum())}

    cap, thr = 12000, 4.0
    pairs = [noisy_pair(rng, 0.5) for _ in range(n)]
    sx, sy, dx, dy, mt = ([t(p[i]) for p in pairs] for i in range(5))
    d_nA = [torch.tensor([cap], dtype=torch.int32, device=dev) for _ in range(n)]
    rws = nm.RansacBatchWorkspace(n, cap, 4096, dev)
    with torch.cuda.stream(stream):
        Hb, _, _, status = nm.ransac_batch_dev(2, sx, sy, d_nA, dx, dy, mt, iterations=4096, threshold=thr,
                                               seeds=list(range(n)), capA=cap, workspace=rws)
    torch.cuda.synchronize()
    runs = {"refit": lambda: nm.ransac_refit_batch_dev(2, sx, sy, d_nA, dx, dy, mt, Hb, status=status, rounds=2,
                                                       threshold=thr, capA=cap)}
    for s in strides:
        runs["verify_stride%d" % s] = (lambda s=s: verify(s))
    sp = karms.spread(karms.time_eager(runs, stream, a.rounds, a.warmup))
    med = sp["median_us"]
    must = {"verify_stride%d" % s: n * 4 * ((FW // s) * (FH // s) + FW * FH) for s in strides}
    karms.emit({"tool": "klink_verify", "pairs": n, "frame": [FW, FH], "rounds": a.rounds, **sp, "bytes_to_move": must,
                "gb_per_s": {k: must[k] / med[k] / 1e3 for k in must}, "checks": stats})


if __name__ == "__main__":
    main()
