"""What homography-guided matching (nm_sift_match_guided_batch_dev_f32) costs beside the blind match call it follows, on the GPU.

    python tools/kguided.py [--pairs 16] [--rows 12000] [--rounds 20] [--radius2 9] [--trace]

Input: `pairs` frame pairs of `rows` x `rows` keypoints spread over 1920 x 1080. 60 % of B's rows are A's rows moved by a
homography with 0.4 px of noise and carry A's descriptor with noise, the rest are unrelated. The blind match, the batched
RANSAC (2 048 hypotheses) and two refit rounds give H, as a client would have it. One round = sift_match_batch_dev, then
the guided call on the same pairs, each bracketed by device events on one stream; rounds alternate the two after warm-up.
The guided call's outputs are checked against its host twin before timing. Prints one JSON line: medians with min-max and
their ratio. --trace runs only a few match + guided calls (for `rocprofv3 --kernel-trace --stats`: launches, kernel times).
"""
import argparse
import os

import numpy as np

import karms
import torch

import niftymatch_amd as nm

TRUE_H = np.array([[0.995, 0.02, 9.0], [-0.015, 1.005, -6.0], [1.5e-5, -1e-5, 1.0]], np.float64)


def make_pair(rng, rows, shared=0.6, noise=0.4):
    desc = lambda n: np.minimum(np.abs(rng.normal(0, 45, (n, 128))), 255).astype(np.float32)
    A = desc(rows)
    ax, ay = rng.uniform(0, 1920, rows).astype(np.float32), rng.uniform(0, 1080, rows).astype(np.float32)
    B = desc(rows)
    bx, by = rng.uniform(0, 1920, rows).astype(np.float32), rng.uniform(0, 1080, rows).astype(np.float32)
    src = rng.permutation(rows)[:int(shared * rows)]
    dst = rng.permutation(rows)[:len(src)]
    p = TRUE_H @ np.stack([ax[src], ay[src], np.ones(len(src))])
    bx[dst] = (p[0] / p[2] + rng.normal(0, noise, len(src))).astype(np.float32)
    by[dst] = (p[1] / p[2] + rng.normal(0, noise, len(src))).astype(np.float32)
    B[dst] = np.maximum(A[src] + rng.normal(0, 12, (len(src), 128)), 0).astype(np.float32)
    return A, ax, ay, B, bx, by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--rows", type=int, default=12000)
    ap.add_argument("--radius2", type=float, default=9.0)
    karms.timing_args(ap, rounds=20, warmup=3, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kguided.py measures on a GPU"
    dev = torch.device("cuda:0")
    n, cap = a.pairs, a.rows
    rng = np.random.default_rng(0)
    pairs = [make_pair(rng, cap) for _ in range(n)]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    A, ax, ay, B, bx, by = ([t(p[i]) for p in pairs] for i in range(6))
    d_n = [torch.tensor([cap], dtype=torch.int32, device=dev) for _ in range(n)]
    blind = [torch.full((cap,), -1, dtype=torch.int32, device=dev) for _ in range(n)]
    gres = [torch.full((cap,), -1, dtype=torch.int32, device=dev) for _ in range(n)]
    mws = nm.MatchBatchDevWorkspace(n, cap, cap, dev)
    stream = torch.cuda.Stream()

    def match():
        nm.sift_match_batch_dev(A, d_n, B, d_n, blind, 0.8, workspace=mws, capA=cap, capB=cap)

    with torch.cuda.stream(stream):
        match()
        Hb, best, pos, status = nm.ransac_batch_dev(2, ax, ay, d_n, bx, by, blind, iterations=2048, threshold=4.0,
                                                    seeds=list(range(n)), capA=cap)
        H, cnt, st, done = nm.ransac_refit_batch_dev(2, ax, ay, d_n, bx, by, blind, Hb, status=status, rounds=2,
                                                     threshold=4.0, capA=cap)

    def guided(**kw):
        return nm.sift_match_guided_batch_dev(A, ax, ay, d_n, B, bx, by, d_n, H, status=st, radius2=a.radius2, capA=cap,
                                              capB=cap, results=gres, **kw)

    if a.trace:
        with torch.cuda.stream(stream):
            for _ in range(5):
                match()
                guided()
        torch.cuda.synchronize()
        karms.emit({"tool": "kguided", "trace_calls": 5, "pairs": n, "rows": cap})
        return

    with torch.cuda.stream(stream):
        _, gcnt, gbest = guided(want_distance=True)
    torch.cuda.synchronize()
    hres, hcnt, hbest = nm.sift_match_guided_host([p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], [cap] * n,
                                                  [p[3] for p in pairs], [p[4] for p in pairs], [p[5] for p in pairs], [cap] * n,
                                                  H.cpu().numpy(), status=st.cpu().numpy(), radius2=a.radius2, capA=cap,
                                                  capB=cap, want_distance=True)
    for k in range(n):
        assert np.array_equal(gres[k].cpu().numpy(), hres[k]), "device and host twin differ (result, pair %d)" % k
        assert np.array_equal(gbest[k].cpu().numpy().view(np.uint32), hbest[k].view(np.uint32)), "best distance, pair %d" % k
    assert np.array_equal(gcnt.cpu().numpy(), hcnt), "device and host twin differ (count)"

    sp = karms.spread(karms.time_eager({"match": match, "guided": guided}, stream, a.rounds, a.warmup))
    med = sp["median_us"]
    karms.emit({"tool": "kguided", "pairs": n, "rows": cap, "radius2": a.radius2, "rounds": a.rounds, **sp,
                "guided_over_match": med["guided"] / med["match"], "library": os.path.basename(nm.LIB_PATH),
                "blind_matches": [int((b >= 0).sum()) for b in blind[:4]],
                "guided_matches": [int(x) for x in hcnt[:4]], "status": [int(x) for x in st.cpu().tolist()][:4]})


if __name__ == "__main__":
    main()
