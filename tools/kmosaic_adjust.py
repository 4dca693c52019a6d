"""What the global mosaic adjustment (nm_mosaic_adjust_dev_f32) costs on the GPU.

    python tools/kmosaic_adjust.py [--rounds 20] [--iterations 5] [--trace]

n = 64 frames on a closed path (the loop of tests/mosaic_adjust_ref.py, walked 64 / 12 times), L = 64 links (the sequential
ones and the closing one, so that every frame is tied to the anchor) and L = 256 (those and 192 between frames two or three
apart drawn at random), capA = 4096 rows per link with 0.3 px noise, a drifted chain. The call alone, bracketed
by device events on one stream, `rounds` times after warm-up. The device outputs are checked against the host twin bit for
bit before timing. Prints one JSON line: medians with min-max per call, launches per call, the end reason and the steps.
--trace runs only a few calls (for `rocprofv3 --kernel-trace --stats`: kernel times per launch; no counters).
"""
import argparse
import os
import sys

import numpy as np

import karms

sys.path.insert(0, os.path.join(karms.ROOT, "tests"))
import torch  # noqa: E402

import niftymatch_amd as nm  # noqa: E402
import mosaic_adjust_ref as R  # noqa: E402

N, CAP = 64, 4096


def problem(L, rng):
    G = np.stack([R.true_maps(12)[k % 12] for k in range(N)])
    la = list(range(N)) + [int(rng.integers(0, N)) for _ in range(L - N)]      # the sequential links and the closing one
    lb = [(a + 1) % N for a in la[:N]] + [(a + int(rng.integers(2, 4))) % N for a in la[N:]]
    cols = [[] for _ in range(7)]
    for a, b in zip(la, lb):
        for c, v in zip(cols, R.link_points(G[a], G[b], rng, CAP - 64, 0.3, 32, CAP)):
            c.append(v)
    chain = []
    for k in range(N):
        D = np.eye(3) + (k > 0) * np.array([[2e-3, -1e-3, 1.5], [1e-3, -2e-3, -1.0], [2e-6, 1e-6, 0]]) * np.sin(1 + k)
        M = np.linalg.inv(G[k] @ D)
        chain.append((M / M[2, 2]).reshape(9))
    return la, lb, cols[:6], np.stack(cols[6]), np.array(chain, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=5)
    karms.timing_args(ap, rounds=20, warmup=3, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kmosaic_adjust.py measures on a GPU"
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    stream = torch.cuda.Stream()
    out = {"tool": "kmosaic_adjust", "frames": N, "capA": CAP, "rounds": a.rounds, "iterations": a.iterations}
    for L in (64, 256):
        la, lb, tab, mask, chain = problem(L, np.random.default_rng(L))
        up = [[t(np.asarray(v)) if k != 2 else t(np.array([v], np.int32)) for v in tab[k]] for k in range(6)]
        d_mask, d_chain = t(mask), t(chain)
        ws = nm.MosaicAdjustWorkspace(N, L, dev)
        kw = dict(iterations=a.iterations, max_step=200.0)

        def call():
            return nm.mosaic_adjust(la, lb, *up, d_chain, R.FW, R.FH, mask=d_mask, workspace=ws, **kw)

        if a.trace:
            with torch.cuda.stream(stream):
                for _ in range(3):
                    call()
            torch.cuda.synchronize()
            continue
        with torch.cuda.stream(stream):
            got = call()
        torch.cuda.synchronize()
        host = nm.mosaic_adjust_host(la, lb, *tab, chain, R.FW, R.FH, mask=mask, **kw)
        for d, h in zip(got, host):
            assert np.array_equal(d.cpu().numpy().view(np.uint8), h.view(np.uint8)), "device and host twin differ"
        sp = karms.spread(karms.time_eager({"call": call}, stream, a.rounds, a.warmup))
        out["L%d" % L] = {"median_us": sp["median_us"]["call"], "min_max_us": sp["min_max_us"]["call"],
                          "launches": (a.iterations + 1) * (-(-L // 64) + 1), "end": int(host[3][7]), "steps": int(host[3][5]),
                          "cost": [float(host[3][0]), float(host[3][1])], "unknown_frames": int(host[3][4])}
    karms.emit(out)


if __name__ == "__main__":
    main()
