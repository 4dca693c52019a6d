"""Batched, device-sampled RANSAC (nm_ransac_batch_dev_f32) against the per-pair path (nm_ransac_f32), on the GPU.

    python tools/kransac_batch.py [--pairs 16] [--iterations 4096] [--rounds 20] [--trace]

Both sides see the same 1080p-like pairs (12 000 source rows, ~5 000 of them matched, 60 % of those on a homography) and
the same sample lists: the per-pair side gets the batched entry's draws as a device rand_list, uploaded before timing. One
round = 16 back-to-back nm_ransac_f32 calls (preallocated outputs, no host work) then one batched call, each bracketed by
device events on one stream; rounds alternate the two after warm-up. Outputs are checked equal before timing. Prints one
JSON line. --trace runs only a few batched calls (for `rocprofv3 --kernel-trace --stats`: launches per call, kernel times).
"""
import argparse
import ctypes as C

import numpy as np

import karms
import torch

import niftymatch_amd as nm

TRUE_H = np.array([[1.02, 0.03, 12.0], [-0.02, 0.98, -7.0], [1e-5, -2e-5, 1.0]])


def sample_rows(V, seed, iterations, S):
    """rand_list[t][s] = V[j] with j drawn by the library's own host twin of the device sampler (nm_ransac_batch_sample),
    so this tool holds no copy of the sampler's specification."""
    draw = nm.lib().nm_ransac_batch_sample
    m = len(V)
    j = np.fromiter((draw(seed, t, s, S, m) for t in range(iterations) for s in range(S)), np.int64, iterations * S)
    assert (j >= 0).all()
    return V[j].reshape(iterations, S).astype(np.int32)


def make_pair(rng, nA=12000, nB=12000, matched=5000, inlier_frac=0.6):
    sx = rng.uniform(0, 1920, nA).astype(np.float32)
    sy = rng.uniform(0, 1080, nA).astype(np.float32)
    dx = rng.uniform(0, 1920, nB).astype(np.float32)
    dy = rng.uniform(0, 1080, nB).astype(np.float32)
    matches = np.full(nA, -1, np.int32)
    rows = rng.permutation(nA)[:matched]
    matches[rows] = rng.permutation(nB)[:matched]
    good = rows[rng.random(matched) < inlier_frac]
    p = TRUE_H @ np.stack([sx[good], sy[good], np.ones(len(good))])
    dx[matches[good]] = (p[0] / p[2]).astype(np.float32)
    dy[matches[good]] = (p[1] / p[2]).astype(np.float32)
    return sx, sy, dx, dy, matches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=4096)
    ap.add_argument("--threshold", type=float, default=4.0)
    karms.timing_args(ap, rounds=20, warmup=3, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kransac_batch.py measures on a GPU"
    dev = torch.device("cuda:0")
    n, it, thr, cap = a.pairs, a.iterations, a.threshold, 12000
    rng = np.random.default_rng(0)
    pairs = [make_pair(rng) for _ in range(n)]
    seeds = list(range(100, 100 + n))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    sx, sy, dx, dy, mt = ([t(p[i]) for p in pairs] for i in range(5))
    d_nA = [torch.tensor([cap], dtype=torch.int32, device=dev) for _ in range(n)]
    ws = nm.RansacBatchWorkspace(n, cap, it, dev)
    stream = torch.cuda.Stream()

    def batched(want_all=False):
        return nm.ransac_batch_dev(2, sx, sy, d_nA, dx, dy, mt, iterations=it, threshold=thr, seeds=seeds, capA=cap,
                                   workspace=ws, want_all=want_all)

    if a.trace:
        with torch.cuda.stream(stream):
            for _ in range(5):
                batched()
        torch.cuda.synchronize()
        karms.emit({"tool": "kransac_batch", "trace_calls": 5, "pairs": n, "iterations": it})
        return

    # the per-pair side: aligned rows (align_points semantics) and the batched entry's sample lists, on the device
    aligned, lists = [], []
    for (psx, psy, pdx, pdy, pm), seed in zip(pairs, seeds):
        ok = (pm >= 0) & (psx >= 0)
        al = [np.where(ok, psx, -1).astype(np.float32), np.where(ok, psy, -1).astype(np.float32),
              np.where(ok, pdx[np.maximum(pm, 0)], -1).astype(np.float32),
              np.where(ok, pdy[np.maximum(pm, 0)], -1).astype(np.float32)]
        aligned.append([t(v) for v in al])
        lists.append(t(sample_rows(np.flatnonzero(ok), seed, it, 4)))
    Ha = [torch.zeros((it, 9), dtype=torch.float32, device=dev) for _ in range(n)]
    inl = [torch.zeros(it, dtype=torch.int32, device=dev) for _ in range(n)]
    Hb = [torch.zeros(9, dtype=torch.float32, device=dev) for _ in range(n)]
    pos = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(n)]
    L = nm.lib()

    def per_pair():
        for k in range(n):
            st = L.nm_ransac_f32(2, *[v.data_ptr() for v in aligned[k]], cap, lists[k].data_ptr(), it, C.c_float(thr),
                                 Ha[k].data_ptr(), inl[k].data_ptr(), Hb[k].data_ptr(), pos[k].data_ptr(),
                                 C.c_void_p(stream.cuda_stream))
            assert st == 0, st

    with torch.cuda.stream(stream):
        per_pair()
        out = batched(want_all=True)
    torch.cuda.synchronize()
    for k in range(n):
        assert int(out[3][k]) == 1 and int(out[2][k]) == int(pos[k].item())
        assert torch.equal(out[4][k].view(torch.int32), Ha[k].view(torch.int32)) and torch.equal(out[5][k], inl[k])
        assert torch.equal(out[0][k].view(torch.int32), Hb[k].view(torch.int32))

    runs = {"per_pair": per_pair, "batched": batched, "batched_all": lambda: batched(True)}
    sp = karms.spread(karms.time_eager(runs, stream, a.rounds, a.warmup))
    med = sp["median_us"]
    karms.emit({"tool": "kransac_batch", "pairs": n, "iterations": it, "rows": cap,
                "matched_rows": [int((p[4] >= 0).sum()) for p in pairs][:2], "rounds": a.rounds, **sp,
                "speedup": med["per_pair"] / med["batched"], "speedup_with_all_outputs": med["per_pair"] / med["batched_all"],
                "best_inliers": [int(x) for x in out[1].cpu().tolist()][:4]})


if __name__ == "__main__":
    main()
