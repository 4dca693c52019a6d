"""What homography-guided matching costs on unsigned-char descriptors (nm_sift_match_guided_u8_batch_dev) beside the fp32
guided call (nm_sift_match_guided_batch_dev_f32) on float copies of the same bytes, on the GPU.

    python tools/kguided_u8.py [--pairs 16] [--rows 12000] [--rounds 20] [--radius2 9] [--trace a|b]

Input: that of tools/kguided.py (`pairs` frame pairs of `rows` x `rows` keypoints over 1920 x 1080, 60 % of B's rows A's
rows moved by a homography), the descriptors finished to u8 by desc_finish_batch_dev. The u8 blind match, the batched RANSAC
(2 048 hypotheses) and two refit rounds give H, as a client of the byte pipeline would have it. Arm (a) is the fp32 guided
call on float copies of the bytes, arm (b) the u8 guided call on the bytes; each is bracketed by device events on one stream
and the rounds alternate the two after warm-up. Before timing, arm (b)'s outputs are checked against arm (a)'s and against
the u8 host twin. Prints one JSON line: medians with min-max, their ratio, and whether (b) lies inside (a)'s spread
(median (b) <= median (a) + max (a) - min (a)). --trace a / --trace b runs a few calls of that arm alone (for
`rocprofv3 --kernel-trace --stats`: launches, kernel times).
"""
import argparse
import os

import numpy as np

import karms
import torch

import niftymatch_amd as nm
from kguided import make_pair


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--rows", type=int, default=12000)
    ap.add_argument("--radius2", type=float, default=9.0)
    ap.add_argument("--trace", choices=("a", "b"))
    karms.timing_args(ap, rounds=20, warmup=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kguided_u8.py measures on a GPU"
    dev = torch.device("cuda:0")
    n, cap = a.pairs, a.rows
    rng = np.random.default_rng(0)
    pairs = [make_pair(rng, cap) for _ in range(n)]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rawA, ax, ay, rawB, bx, by = ([t(p[i]) for p in pairs] for i in range(6))
    d_n = [torch.tensor([cap], dtype=torch.int32, device=dev) for _ in range(n)]
    _, A8 = nm.desc_finish_batch_dev(rawA, d_n, out_u8=True, capacity=cap)
    _, B8 = nm.desc_finish_batch_dev(rawB, d_n, out_u8=True, capacity=cap)
    A32, B32 = [x.float() for x in A8], [x.float() for x in B8]
    del rawA, rawB
    blind = [torch.full((cap,), -1, dtype=torch.int32, device=dev) for _ in range(n)]
    res = {arm: [torch.full((cap,), -1, dtype=torch.int32, device=dev) for _ in range(n)] for arm in "ab"}
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        nm.sift_match_u8_batch_dev(A8, d_n, B8, d_n, results=blind, ambiguity=0.8, capA=cap, capB=cap)
        Hb, best, pos, status = nm.ransac_batch_dev(2, ax, ay, d_n, bx, by, blind, iterations=2048, threshold=4.0,
                                                    seeds=list(range(n)), capA=cap)
        H, cnt, st, done = nm.ransac_refit_batch_dev(2, ax, ay, d_n, bx, by, blind, Hb, status=status, rounds=2,
                                                     threshold=4.0, capA=cap)
    kw = dict(status=st, radius2=a.radius2, capA=cap, capB=cap)
    arms = {"a": lambda **k: nm.sift_match_guided_batch_dev(A32, ax, ay, d_n, B32, bx, by, d_n, H, results=res["a"], **kw, **k),
            "b": lambda **k: nm.sift_match_guided_u8_batch_dev(A8, ax, ay, d_n, B8, bx, by, d_n, H, results=res["b"], **kw, **k)}

    if a.trace:
        with torch.cuda.stream(stream):
            for _ in range(5):
                arms[a.trace]()
        torch.cuda.synchronize()
        karms.emit({"tool": "kguided_u8", "trace_arm": a.trace, "trace_calls": 5, "pairs": n, "rows": cap})
        return

    with torch.cuda.stream(stream):
        _, cnt_a, best_a = arms["a"](want_distance=True)
        _, cnt_b, best_b = arms["b"](want_distance=True)
    torch.cuda.synchronize()
    u32 = lambda x: x.cpu().numpy().view(np.uint32)
    for k in range(n):
        assert torch.equal(res["a"][k], res["b"][k]), "u8 and fp32 guided calls differ (result, pair %d)" % k
        assert np.array_equal(u32(best_a[k]), u32(best_b[k])), "u8 and fp32 guided calls differ (best distance, pair %d)" % k
    assert torch.equal(cnt_a, cnt_b), "u8 and fp32 guided calls differ (count)"
    host = lambda xs: [x.cpu().numpy() for x in xs]
    hres, hcnt, hbest = nm.sift_match_guided_u8_host(host(A8), host(ax), host(ay), [cap] * n, host(B8), host(bx), host(by),
                                                     [cap] * n, H.cpu().numpy(), status=st.cpu().numpy(), radius2=a.radius2,
                                                     capA=cap, capB=cap, want_distance=True)
    for k in range(n):
        assert np.array_equal(res["b"][k].cpu().numpy(), hres[k]), "device and host twin differ (result, pair %d)" % k
        assert np.array_equal(u32(best_b[k]), hbest[k].view(np.uint32)), "device and host twin differ (best, pair %d)" % k
    assert np.array_equal(cnt_b.cpu().numpy(), hcnt), "device and host twin differ (count)"

    sp = karms.spread(karms.time_eager(arms, stream, a.rounds, a.warmup))
    med, (lo, hi) = sp["median_us"], sp["min_max_us"]["a"]
    bar = med["a"] + hi - lo
    karms.emit({"tool": "kguided_u8", "pairs": n, "rows": cap, "radius2": a.radius2, "rounds": a.rounds,
                "arms": {"a": "fp32 guided on float copies", "b": "u8 guided"}, **sp,
                "u8_over_fp32": med["b"] / med["a"], "bar_us": bar, "inside_spread": med["b"] <= bar,
                "library": os.path.basename(nm.LIB_PATH), "blind_matches": [int((b >= 0).sum()) for b in blind[:4]],
                "guided_matches": [int(x) for x in hcnt[:4]], "status": [int(x) for x in st.cpu().tolist()][:4]})


if __name__ == "__main__":
    main()
