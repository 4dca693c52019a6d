"""What the mutual-nearest-neighbour filter (nm_sift_match_mutual_batch_dev_f32) costs beside the second, swapped blind match
it replaces, on the GPU.

    python tools/kmutual.py [--pairs 16] [--rounds 20] [--related] [--trace] [--stats]

Input: `pairs` frame pairs of the bench's synthetic 1080p frames (uniform noise, Gaussian pre-blur; about 12k keypoints
each), detected once. Pair p is frames (2p, 2p + 1) as in bench.py; with --related the second frame of a pair is the first one
moved by (9, 5) pixels and mixed with a quarter of another noise frame, so that the ratio test accepts a large share of rows.
Arms, each bracketed by device events on one stream and alternated round by round after warm-up:
    a  sift_match_batch_dev(A, B), then sift_match_batch_dev(B, A): what a client must run for a cross-check without this
       entry (the comparison of the two lists on the host is not even timed);
    b  sift_match_batch_dev(A, B), then sift_match_mutual_batch_dev;
    m  the mutual call alone (on the match list of the warm-up).
Pair 0's device outputs are checked against the host twin before timing. Prints one JSON line: medians with min-max, the
share of matches the filter removes. --trace runs only a few match + mutual calls (for `rocprofv3 --kernel-trace --stats`:
launches, kernel times). --stats reads the two counters a scratch build writes
(python tools/build_variant.py mstats nm_match_mutual.hip -DNMM_STATS=1; NM_DIAGNOSTIC=1
NM_HIP_LIB=tools/_variants/libnm_hip_mstats.so): (claim, row) pairs scanned and 16-dimension chunks walked.
"""
import argparse
import os

import numpy as np

import karms
import torch

import niftymatch_amd as nm
from niftymatch_amd import synth

W, H, CAP = 1920, 1080, 16384


def make_frames(dev, n, related):
    taps, r = nm.create_kernel_for_sigma(synth.preblur_sigma(W, H))
    taps_d = torch.from_numpy(taps).to(dev)
    frame = lambda s: nm.convolve(synth.noise_frame_torch(s, W, H, dev), taps_d, r)
    out = []
    for p in range(n):
        a = frame(2 * p)
        b = frame(2 * p + 1)
        if related:
            b = (0.75 * torch.roll(a, (5, 9), (0, 1)) + 0.25 * b).contiguous()
        out += [a, b]
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--related", action="store_true")
    ap.add_argument("--stats", action="store_true")
    karms.timing_args(ap, rounds=20, warmup=3, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kmutual.py measures on a GPU"
    assert 1 <= a.pairs <= nm.MATCH_MAX_BATCH
    dev = torch.device("cuda:0")
    n = a.pairs
    frames = make_frames(dev, n, a.related)
    arenas = [nm.SiftArena(W, H, CAP, device=dev) for _ in range(2 * n)]
    for c in range(0, 2 * n, 16):
        nm.detect_describe_batch(arenas[c:c + 16], frames[c:c + 16])
    torch.cuda.synchronize()
    del frames
    A, B = arenas[0::2], arenas[1::2]
    dA, dB, nA, nB = [x.desc for x in A], [x.desc for x in B], [x.num_items for x in A], [x.num_items for x in B]
    full = lambda: [torch.full((CAP,), -1, dtype=torch.int32, device=dev) for _ in range(n)]
    fwd, rev, mres = full(), full(), full()
    mws = nm.MatchBatchDevWorkspace(n, CAP, CAP, dev)
    uws = nm.MatchMutualWorkspace(n, CAP, dev)
    stream = torch.cuda.Stream()

    def match():
        nm.sift_match_batch_dev(dA, nA, dB, nB, fwd, 0.8, workspace=mws, capA=CAP, capB=CAP)

    def swapped():
        nm.sift_match_batch_dev(dB, nB, dA, nA, rev, 0.8, workspace=mws, capA=CAP, capB=CAP)

    def mutual(**kw):
        return nm.sift_match_mutual_batch_dev(dA, nA, dB, nB, fwd, capA=CAP, capB=CAP, results=mres, workspace=uws, **kw)

    if a.trace:
        with torch.cuda.stream(stream):
            for _ in range(5):
                match()
                mutual()
        torch.cuda.synchronize()
        karms.emit({"tool": "kmutual", "trace_calls": 5, "pairs": n, "related": a.related})
        return

    with torch.cuda.stream(stream):
        match()
        if a.stats:
            uws.buf[:512].zero_()
        _, mcnt, mfwd = mutual(want_distance=True)
    torch.cuda.synchronize()
    rows = [int(x.item()) for x in nA]
    claims = [int((f >= 0).sum()) for f in fwd]
    kept = [int(x) for x in mcnt.cpu().tolist()]
    out = {"tool": "kmutual", "pairs": n, "related": a.related, "library": os.path.basename(nm.LIB_PATH),
           "rows_A": rows[:4], "rows_B": [int(x.item()) for x in nB][:4], "claims": claims[:4], "kept": kept[:4],
           "claim_share_of_rows": sum(claims) / max(sum(rows), 1), "removed_share_of_claims": 1.0 - sum(kept) / max(sum(claims), 1)}
    if a.stats:
        st = uws.buf[256:272].cpu().numpy().view(np.uint64)
        out["stats"] = {"claim_row_pairs": int(st[0]), "chunks": int(st[1]),
                        "mean_chunks_per_pair": float(st[1]) / max(float(st[0]), 1.0)}
        karms.emit(out)
        return
    hres, hcnt, hfwd = nm.sift_match_mutual_host([dA[0].cpu().numpy()], [rows[0]], [dB[0].cpu().numpy()], [int(nB[0].item())],
                                                 [fwd[0].cpu().numpy()], capA=CAP, capB=CAP, want_distance=True)
    assert np.array_equal(mres[0].cpu().numpy(), hres[0]), "device and host twin differ (result, pair 0)"
    assert np.array_equal(mfwd[0].cpu().numpy().view(np.uint32), hfwd[0].view(np.uint32)), "forward distance, pair 0"
    assert kept[0] == int(hcnt[0]), "device and host twin differ (count)"

    arms = {"a_match_then_swapped_match": lambda: (match(), swapped()), "b_match_then_mutual": lambda: (match(), mutual()),
            "match_alone": match, "swapped_match_alone": swapped, "mutual_alone": mutual}
    sp = karms.spread(karms.time_eager(arms, stream, a.rounds, a.warmup))
    med = sp["median_us"]
    out.update({"rounds": a.rounds, **sp, "b_over_a": med["b_match_then_mutual"] / med["a_match_then_swapped_match"],
                "mutual_over_swapped_match": med["mutual_alone"] / med["swapped_match_alone"]})
    karms.emit(out)
    for x in arenas:
        x.close()


if __name__ == "__main__":
    main()
