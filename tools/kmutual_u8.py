"""What the mutual filter for u8 descriptors (nm_sift_match_mutual_u8_batch_dev) costs beside the second, swapped u8 match it
replaces, and beside the fp32 matcher with the fp32 filter on float copies of the same bytes, on the GPU.

    python tools/kmutual_u8.py [--pairs 16] [--rounds 20] [--related] [--trace]

Input: `pairs` frame pairs of the bench's synthetic 1080p frames (uniform noise, Gaussian pre-blur; about 12k keypoints
each), detected once and finished once (NM_DESC_L2, u8 output). Pair p is frames (2p, 2p + 1) as in bench.py; with --related
the second frame of a pair is the first one moved by (9, 5) pixels and mixed with a quarter of another noise frame, so that
the ratio test accepts a large share of rows. Arms, each bracketed by device events on one stream and alternated round by
round after warm-up:
    a  sift_match_u8_batch_dev(A, B), then sift_match_u8_batch_dev(B, A): what a byte client must run for a cross-check
       without this entry (the comparison of the two lists on the host is not even timed);
    b  sift_match_u8_batch_dev(A, B), then sift_match_mutual_u8_batch_dev;
    c  sift_match_batch_dev, then sift_match_mutual_batch_dev, on float copies of the same bytes;
    and alone: the u8 match, the swapped u8 match, the mutual u8 call (on the match list of the warm-up).
Before timing, pair 0's device outputs are checked against the host twin and every pair's outputs against the fp32 filter on
float copies (result, count and forward distance, bit for bit). Prints one JSON line: medians with min-max, claims / rows and
the share of claims the filter removes. --trace runs only a few calls of each arm (for a kernel trace in a run of its own,
without counters).
"""
import argparse

import numpy as np

import karms
import torch

import niftymatch_amd as nm

from kmutual import CAP, H, W, make_frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--related", action="store_true")
    karms.timing_args(ap, rounds=20, warmup=3, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kmutual_u8.py measures on a GPU"
    assert 1 <= a.pairs <= nm.MATCH_MAX_BATCH
    dev = torch.device("cuda:0")
    n = a.pairs
    frames = make_frames(dev, n, a.related)
    arenas = [nm.SiftArena(W, H, CAP, device=dev) for _ in range(2 * n)]
    for c in range(0, 2 * n, 16):
        nm.detect_describe_batch(arenas[c:c + 16], frames[c:c + 16])
    torch.cuda.synchronize()
    del frames
    counts = [x.num_items for x in arenas]
    u8 = [torch.zeros((CAP, 128), dtype=torch.uint8, device=dev) for _ in range(2 * n)]
    nm.desc_finish_batch_dev([x.desc for x in arenas], counts, out_u8=u8, capacity=CAP)
    torch.cuda.synchronize()
    flt = [u.float() for u in u8]
    uA, uB, fA, fB, nA, nB = u8[0::2], u8[1::2], flt[0::2], flt[1::2], counts[0::2], counts[1::2]
    full = lambda: [torch.full((CAP,), -1, dtype=torch.int32, device=dev) for _ in range(n)]
    fwd, rev, mres, ffwd, fres = full(), full(), full(), full(), full()
    uws = nm.MatchU8Workspace(n, CAP, CAP, dev)
    mws = nm.MatchMutualU8Workspace(n, CAP, CAP, dev)
    bws = nm.MatchBatchDevWorkspace(n, CAP, CAP, dev)
    fws = nm.MatchMutualWorkspace(n, CAP, dev)
    stream = torch.cuda.Stream()

    def match():
        nm.sift_match_u8_batch_dev(uA, nA, uB, nB, results=fwd, ambiguity=0.8, workspace=uws, capA=CAP, capB=CAP)

    def swapped():
        nm.sift_match_u8_batch_dev(uB, nB, uA, nA, results=rev, ambiguity=0.8, workspace=uws, capA=CAP, capB=CAP)

    def mutual(**kw):
        return nm.sift_match_mutual_u8_batch_dev(uA, nA, uB, nB, fwd, capA=CAP, capB=CAP, results=mres, workspace=mws, **kw)

    def match_f32():
        nm.sift_match_batch_dev(fA, nA, fB, nB, ffwd, 0.8, workspace=bws, capA=CAP, capB=CAP)

    def mutual_f32(**kw):
        return nm.sift_match_mutual_batch_dev(fA, nA, fB, nB, ffwd, capA=CAP, capB=CAP, results=fres, workspace=fws, **kw)

    if a.trace:
        with torch.cuda.stream(stream):
            for _ in range(5):
                match()
                swapped()
                mutual()
                match_f32()
                mutual_f32()
        torch.cuda.synchronize()
        karms.emit({"tool": "kmutual_u8", "trace_calls": 5, "pairs": n, "related": a.related})
        return

    with torch.cuda.stream(stream):
        match()
        match_f32()
        _, mcnt, mfwd = mutual(want_distance=True)
        _, fcnt, ffd = mutual_f32(want_distance=True)
    torch.cuda.synchronize()
    rows = [int(x.item()) for x in nA]
    hres, hcnt, hfwd = nm.sift_match_mutual_u8_host([uA[0].cpu().numpy()], [rows[0]], [uB[0].cpu().numpy()], [int(nB[0].item())],
                                                    [fwd[0].cpu().numpy()], capA=CAP, capB=CAP, want_distance=True)
    assert np.array_equal(mres[0].cpu().numpy(), hres[0]), "device and host twin differ (result, pair 0)"
    assert np.array_equal(mfwd[0].cpu().numpy().view(np.uint32), hfwd[0].view(np.uint32)), "forward distance, pair 0"
    assert int(mcnt[0].item()) == int(hcnt[0]), "device and host twin differ (count)"
    assert torch.equal(mcnt, fcnt), "u8 filter and fp32 filter on float copies differ (count)"
    for k in range(n):
        assert torch.equal(fwd[k], ffwd[k]), "u8 matcher and fp32 matcher on float copies differ (pair %d)" % k
        assert torch.equal(mres[k], fres[k]), "u8 filter and fp32 filter on float copies differ (result, pair %d)" % k
        assert torch.equal(mfwd[k].view(torch.int32), ffd[k].view(torch.int32)), "forward distance, pair %d" % k
    claims = [int((f >= 0).sum()) for f in fwd]
    kept = [int(x) for x in mcnt.cpu().tolist()]
    out = {"tool": "kmutual_u8", "pairs": n, "related": a.related, "rows_A": rows[:4], "rows_B": [int(x.item()) for x in nB][:4],
           "claims": claims[:4], "kept": kept[:4], "claim_share_of_rows": sum(claims) / max(sum(rows), 1),
           "removed_share_of_claims": 1.0 - sum(kept) / max(sum(claims), 1)}

    arms = {"a_match_u8_then_swapped_match_u8": lambda: (match(), swapped()), "b_match_u8_then_mutual_u8": lambda: (match(), mutual()),
            "c_match_f32_then_mutual_f32": lambda: (match_f32(), mutual_f32()), "match_u8_alone": match,
            "swapped_match_u8_alone": swapped, "mutual_u8_alone": mutual}
    sp = karms.spread(karms.time_eager(arms, stream, a.rounds, a.warmup))
    med = sp["median_us"]
    out.update({"rounds": a.rounds, **sp,
                "b_over_a": med["b_match_u8_then_mutual_u8"] / med["a_match_u8_then_swapped_match_u8"],
                "b_over_c": med["b_match_u8_then_mutual_u8"] / med["c_match_f32_then_mutual_f32"],
                "mutual_u8_over_swapped_match_u8": med["mutual_u8_alone"] / med["swapped_match_u8_alone"],
                "mutual_u8_us_per_pair": med["mutual_u8_alone"] / n})
    karms.emit(out)
    for x in arenas:
        x.close()


if __name__ == "__main__":
    main()
