"""What the inlier refit (nm_ransac_refit_batch_dev_f32) adds to the batched RANSAC call it follows, on the GPU.

    python tools/kransac_refit.py [--pairs 16] [--iterations 4096] [--refit-rounds 2] [--rounds 20] [--trace]

The input is tools/kransac_batch.py's: 16 pairs of 12 000 source rows, ~5 000 of them matched, 60 % of those on a homography
(here with 0.5 px of noise, so that the refit has something to average), 4 096 homography hypotheses. One round = the
batched RANSAC call alone, then RANSAC + refit, then the refit alone on the last H_best, each bracketed by device events on
one stream; rounds alternate the three after warm-up. The refit's outputs are checked against its host twin before timing.
Prints one JSON line: medians with min-max, and `added_us` = median(RANSAC + refit) - median(RANSAC). --trace runs only a
few RANSAC + refit calls (for `rocprofv3 --kernel-trace --stats`: launches per call, kernel times).
"""
import argparse
import statistics

import numpy as np

import karms
import torch

import niftymatch_amd as nm

from kransac_batch import TRUE_H, make_pair


def noisy_pair(rng, sigma):
    sx, sy, dx, dy, matches = make_pair(rng)
    rows = np.flatnonzero(matches >= 0)
    p = TRUE_H @ np.stack([sx[rows], sy[rows], np.ones(len(rows))])
    on = (np.abs(dx[matches[rows]] - (p[0] / p[2]).astype(np.float32)) < 1e-3)
    dx[matches[rows[on]]] += rng.normal(0, sigma, int(on.sum())).astype(np.float32)
    dy[matches[rows[on]]] += rng.normal(0, sigma, int(on.sum())).astype(np.float32)
    return sx, sy, dx, dy, matches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=4096)
    ap.add_argument("--refit-rounds", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=4.0)
    ap.add_argument("--noise", type=float, default=0.5)
    karms.timing_args(ap, rounds=20, warmup=3, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kransac_refit.py measures on a GPU"
    dev = torch.device("cuda:0")
    n, it, thr, cap, rr = a.pairs, a.iterations, a.threshold, 12000, a.refit_rounds
    rng = np.random.default_rng(0)
    pairs = [noisy_pair(rng, a.noise) for _ in range(n)]
    seeds = list(range(100, 100 + n))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    sx, sy, dx, dy, mt = ([t(p[i]) for p in pairs] for i in range(5))
    d_nA = [torch.tensor([cap], dtype=torch.int32, device=dev) for _ in range(n)]
    ws = nm.RansacBatchWorkspace(n, cap, it, dev)
    stream = torch.cuda.Stream()
    last = {}

    def ransac():
        last["r"] = nm.ransac_batch_dev(2, sx, sy, d_nA, dx, dy, mt, iterations=it, threshold=thr, seeds=seeds, capA=cap,
                                        workspace=ws)
        return last["r"]

    def refit(Hb, status, **kw):
        return nm.ransac_refit_batch_dev(2, sx, sy, d_nA, dx, dy, mt, Hb, status=status, rounds=rr, threshold=thr, capA=cap, **kw)

    def both():
        Hb, best, pos, status = ransac()
        return refit(Hb, status)

    if a.trace:
        with torch.cuda.stream(stream):
            for _ in range(5):
                both()
        torch.cuda.synchronize()
        karms.emit({"tool": "kransac_refit", "trace_calls": 5, "pairs": n, "iterations": it, "refit_rounds": rr})
        return

    with torch.cuda.stream(stream):
        Hb, best, pos, status = ransac()
        out = refit(Hb, status, want_mask=True, want_rms=True)
    torch.cuda.synchronize()
    host = nm.ransac_refit_host(2, [p[0] for p in pairs], [p[1] for p in pairs], [cap] * n, [p[2] for p in pairs],
                                [p[3] for p in pairs], [p[4] for p in pairs], Hb.cpu().numpy(), status=status.cpu().numpy(),
                                rounds=rr, threshold=thr, capA=cap, want_mask=True, want_rms=True)
    for d, h in zip(out, host):
        d = d.cpu().numpy()
        assert np.array_equal(d.view(np.uint32) if d.dtype == np.float32 else d,
                              h.view(np.uint32) if h.dtype == np.float32 else h), "device and host twin differ"
    def corner(H):
        c = np.array([[0, 1920, 0, 1920], [0, 0, 1080, 1080], [1, 1, 1, 1]], np.float64)
        q, g = H.reshape(3, 3).astype(np.float64) @ c, TRUE_H @ c
        return float(np.hypot(q[0] / q[2] - g[0] / g[2], q[1] / q[2] - g[1] / g[2]).max())

    err_in = [corner(h) for h in Hb.cpu().numpy()]
    err_out = [corner(h) for h in out[0].cpu().numpy()]

    runs = {"ransac": ransac, "ransac_refit": both, "refit": lambda: refit(last["r"][0], last["r"][3]),
            "refit_mask_rms": lambda: refit(last["r"][0], last["r"][3], want_mask=True, want_rms=True)}
    sp = karms.spread(karms.time_eager(runs, stream, a.rounds, a.warmup))
    med = sp["median_us"]
    karms.emit({"tool": "kransac_refit", "pairs": n, "iterations": it, "rows": cap, "refit_rounds": rr, "rounds": a.rounds, **sp,
                "added_us": med["ransac_refit"] - med["ransac"],
                "added_over_ransac": (med["ransac_refit"] - med["ransac"]) / med["ransac"],
                "rounds_done": [int(x) for x in out[3].cpu().tolist()],
                "inliers_in_out": [[int(x) for x in best.cpu().tolist()][:4], [int(x) for x in out[1].cpu().tolist()][:4]],
                "corner_error_px_in_out": [float(statistics.median(err_in)), float(statistics.median(err_out))]})


if __name__ == "__main__":
    main()
