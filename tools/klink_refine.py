"""What the direct link refinement (nm_link_refine_batch_dev_f32) costs beside the verification call it precedes, on the GPU.

    python tools/klink_refine.py [--pairs 16] [--rounds 20] [--iterations 4] [--trace]

16 pairs of 1920 x 1080 gray planes (17 frames cut from one textured plane, frame k + 1 is B of pair k and A of pair k + 1,
each the one before shifted by a few pixels and brightened; the starts are the true maps moved by 1.5 px, so every pair
walks all its iterations) at strides 1, 2 and 4 with the homography model, and the verification call on the same pairs,
each bracketed by device events on one stream; rounds alternate the six after warm-up. The device outputs are checked
against the host twin bit for bit before timing. Prints one JSON line: medians with min-max per call and per iteration,
the verification's beside them, and per stride the bytes one iteration must move (A's lattice values and their four
neighbours, 4 bytes each, plus B's gathered lines: every 64-byte line of B that holds a tap, which at strides 1 to 4 is
all of B) so that the time can be set against tools/hbm_probe.py's bandwidth. --trace runs only a few calls (for
`rocprofv3 --kernel-trace --stats`: launches per call, kernel times; no counters).
"""
import argparse

import numpy as np

import karms
import torch

import niftymatch_amd as nm

FW, FH = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=4)
    karms.timing_args(ap, rounds=20, warmup=3, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "klink_refine.py measures on a GPU"
    dev = torch.device("cuda:0")
    n, its = a.pairs, a.iterations
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:FH + 64, 0:FW + 4 * n + 64]
    base = (110 + 45 * np.sin(xx / 9.0) * np.cos(yy / 11.0) + 30 * np.sin((xx + 2 * yy) / 23.0) +
            20 * rng.random(xx.shape)).astype(np.float32)
    frames = [np.ascontiguousarray(base[3 * (k % 2):3 * (k % 2) + FH, 4 * k:4 * k + FW]) for k in range(n + 1)]
    frames = [np.clip((1 + 0.01 * (k % 5)) * f + k % 3, 0, 255).astype(np.float32) for k, f in enumerate(frames)]
    H = np.stack([np.array([1, 0, -4 + 1.2, 0, 1, 3 * (k % 2) - 3 * ((k + 1) % 2) - 0.9, 0, 0, 1], np.float32)
                  for k in range(n)])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_frames, d_H = [t(f) for f in frames], t(H)
    ws, vws = nm.LinkRefineWorkspace(n, dev), nm.LinkVerifyWorkspace(n, dev)
    stream = torch.cuda.Stream()
    strides = (1, 2, 4)
    kw = dict(model=nm.LINK_REFINE_HOMOGRAPHY, iterations=its, max_step=8.0)

    def refine(s):
        return nm.link_refine_batch_dev(d_frames[:-1], d_frames[1:], d_H, stride=s, workspace=ws, **kw)

    def verify(s):
        return nm.link_verify_batch_dev(d_frames[:-1], d_frames[1:], d_H, stride=s, workspace=vws)

    if a.trace:
        with torch.cuda.stream(stream):
            for _ in range(5):
                for s in strides:
                    refine(s)
        torch.cuda.synchronize()
        karms.emit({"tool": "klink_refine", "trace_calls": 5 * len(strides), "pairs": n, "iterations": its})
        return

    checks = {}
    for s in strides:
        with torch.cuda.stream(stream):
            out = refine(s)
        torch.cuda.synchronize()
        host = nm.link_refine_host(frames[:-1], frames[1:], H, stride=s, **kw)
        for d, h in zip(out, host):
            assert np.array_equal(d.cpu().numpy().view(np.uint8), h.view(np.uint8)), "device and host twin differ"
        truth = H.copy()
        truth[:, 2] -= 1.2
        truth[:, 5] += 0.9
        checks[s] = {"walks_min": int(host[2][:, 6].min()), "refined": int(host[1].sum()),
                     "ends": sorted(set(host[2][:, 8].astype(int).tolist())),
                     "shift_error_max_px": float(np.abs(host[0][:, [2, 5]] - truth[:, [2, 5]]).max())}

    runs = {}
    for s in strides:
        runs["refine_stride%d" % s] = (lambda s=s: refine(s))
        runs["verify_stride%d" % s] = (lambda s=s: verify(s))
    sp = karms.spread(karms.time_eager(runs, stream, a.rounds, a.warmup))
    must = {"refine_stride%d" % s: n * 4 * (5 * (FW // s) * (FH // s) + FW * FH) for s in strides}
    per_it = {k: sp["median_us"][k] / its for k in must}
    karms.emit({"tool": "klink_refine", "pairs": n, "frame": [FW, FH], "rounds": a.rounds, "iterations": its, **sp,
                "per_iteration_us": per_it, "bytes_per_iteration": must,
                "gb_per_s": {k: must[k] / per_it[k] / 1e3 for k in must}, "checks": checks})


if __name__ == "__main__":
    main()
