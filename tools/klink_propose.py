"""What the all-pairs vote scan (nm_link_votes_dev_u8) costs beside the route a client has without it: the n (n - 1) directed
frame pairs through nm_sift_match_u8_batch_dev, 64 per call, and a count of each result table, on the GPU.

    python tools/klink_propose.py [--frames 64] [--caps 512,1024,2048] [--rounds 20] [--related] [--splits 0,1] [--trace]

Input: `frames` of the bench's synthetic 1080p frames (uniform noise, Gaussian pre-blur; about 12k keypoints each), detected
and finished once (NM_DESC_L2, u8 output); a frame's first `cap` rows are its descriptors. With --related frame k is frame 0
moved by k (9, 5) pixels and mixed with a quarter of its own noise frame, so that frames overlap and rows pass the ratio test.
Arms, each bracketed by device events on one stream and alternated round by round after warm-up, per cap:
    a        for each group of 64 directed pairs one sift_match_u8_batch_dev call into the rows of one (64, cap) table
             pre-filled with -1, and one count of the table's non-negative entries per row (torch: a compare and a sum):
             ceil(n (n - 1) / 64) calls, twice as many matcher launches;
    b        link_votes_dev: two launches;
    b_zN     the same with the candidate frames of a wave divided into N parts (--splits; 0 is the default rule);
    *_graph  each of the above captured into a HIP graph once and replayed, which leaves the host's issue time of the binding
             out of the comparison.
Before timing, arm b's votes (under every split) are checked against arm a's counts for equality. Prints one JSON line per
cap: medians with min-max in microseconds and b / a. --trace runs a few calls of arms a and b only (for a kernel trace in a
run of its own, without counters).
"""
import argparse
import statistics

import numpy as np

import karms
import torch

import niftymatch_amd as nm
from niftymatch_amd import synth

W, H, CAP = 1920, 1080, 16384
GROUP = 64


def finished_frames(dev, n, related):
    """n (CAP, 128) uint8 tensors of finished descriptors and their device counts, detected 16 frames at a time."""
    taps, r = nm.create_kernel_for_sigma(synth.preblur_sigma(W, H))
    taps_d = torch.from_numpy(taps).to(dev)
    frame = lambda s: nm.convolve(synth.noise_frame_torch(s, W, H, dev), taps_d, r)
    base = frame(0)
    arenas = [nm.SiftArena(W, H, CAP, device=dev) for _ in range(min(n, 16))]
    u8 = [torch.zeros((CAP, 128), dtype=torch.uint8, device=dev) for _ in range(n)]
    counts = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(n)]
    for c in range(0, n, 16):
        ks = list(range(c, min(c + 16, n)))
        frames = [(0.75 * torch.roll(base, (5 * k, 9 * k), (0, 1)) + 0.25 * frame(k)).contiguous() if related and k else frame(k)
                  for k in ks]
        nm.detect_describe_batch(arenas[:len(ks)], frames)
        nm.desc_finish_batch_dev([x.desc for x in arenas[:len(ks)]], [x.num_items for x in arenas[:len(ks)]],
                                 out_u8=[u8[k] for k in ks], capacity=CAP)
        for x, k in zip(arenas, ks):
            counts[k].copy_(x.num_items.reshape(1))
        torch.cuda.synchronize()
    for x in arenas:
        x.close()
    return u8, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--caps", default="512,1024,2048")
    ap.add_argument("--splits", default="0,1")
    ap.add_argument("--related", action="store_true")
    karms.timing_args(ap, rounds=20, warmup=3, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "klink_propose.py measures on a GPU"
    n = a.frames
    assert 2 <= n <= nm.LINK_PROPOSE_MAX_FRAMES
    caps, splits = [int(c) for c in a.caps.split(",")], [int(z) for z in a.splits.split(",")]
    dev = torch.device("cuda:0")
    u8, counts = finished_frames(dev, n, a.related)
    pairs = [(x, y) for x in range(n) for y in range(n) if x != y]
    groups = [pairs[g:g + GROUP] for g in range(0, len(pairs), GROUP)]
    stream = torch.cuda.Stream()

    for cap in caps:
        tables = [torch.empty((len(g), cap), dtype=torch.int32, device=dev) for g in groups]
        pair_counts = [torch.empty(len(g), dtype=torch.int64, device=dev) for g in groups]
        uws = nm.MatchU8Workspace(GROUP, cap, cap, dev)
        lws = nm.LinkVotesWorkspace(n, cap, dev)
        votes = torch.empty((n, n), dtype=torch.int32, device=dev)
        lists = [([u8[x] for x, _ in g], [counts[x] for x, _ in g], [u8[y] for _, y in g], [counts[y] for _, y in g], list(t))
                 for g, t in zip(groups, tables)]

        def arm_a():
            for (A, nA, B, nB, rows), t, pc in zip(lists, tables, pair_counts):
                t.fill_(-1)
                nm.sift_match_u8_batch_dev(A, nA, B, nB, results=rows, ambiguity=0.8, workspace=uws, capA=cap, capB=cap)
                torch.sum(t >= 0, dim=1, out=pc)

        def arm_b(z=0):
            nm.link_votes_set_split(z)
            nm.link_votes_dev(u8, counts, ambiguity=0.8, votes=votes, workspace=lws, cap=cap)
            nm.link_votes_set_split(0)

        if a.trace:
            with torch.cuda.stream(stream):
                for _ in range(3):
                    arm_a()
                    arm_b()
            torch.cuda.synchronize()
            karms.emit({"tool": "klink_propose", "trace_calls": 3, "frames": n, "cap": cap, "related": a.related})
            continue

        with torch.cuda.stream(stream):
            arm_a()
        torch.cuda.synchronize()
        want = np.zeros((n, n), np.int64)
        for g, pc in zip(groups, pair_counts):
            for (x, y), v in zip(g, pc.cpu().tolist()):
                want[x, y] = v
        for z in splits:
            votes.fill_(-1)
            with torch.cuda.stream(stream):
                arm_b(z)
            torch.cuda.synchronize()
            assert np.array_equal(votes.cpu().numpy(), want), "votes and the matcher's pair counts differ (cap %d, split %d)" % (cap, z)

        arms = {"a": arm_a, "b": arm_b}
        arms.update({"b_z%d" % z: (lambda z=z: arm_b(z)) for z in splits if z != 0})
        graphs, kept = karms.capture(arms, stream)                    # the same arms as replays of a captured graph,
        arms.update({name + "_graph": g.replay for name, g in graphs.items()})    # timed by the eager method beside them
        sp = karms.spread(karms.time_eager(arms, stream, a.rounds, a.warmup))
        med = sp["median_us"]
        rows = [min(int(c.item()), cap) for c in counts]
        off = want[~np.eye(n, dtype=bool)]
        karms.emit({"tool": "klink_propose", "frames": n, "cap": cap, "related": a.related, "rows_min_max": [min(rows), max(rows)],
                    "pairs": len(pairs), "votes_min_median_max": [int(off.min()), float(statistics.median(off.tolist())), int(off.max())],
                    "launches": {"a_matcher": 2 * len(groups), "a_calls": len(groups), "b": 2}, "rounds": a.rounds, **sp,
                    "b_over_a": med["b"] / med["a"], "b_graph_over_a_graph": med["b_graph"] / med["a_graph"]})


if __name__ == "__main__":
    main()
