"""Gray pyramid and KLT tracker (nm_gray_pyramid_batch_f32, nm_klt_track_batch_dev_f32) on the GPU, timed as graph replays beside
the stage the tracker stands in for on consecutive frames, the blind matcher nm_sift_match_batch_dev_f32.

    python tools/kklt.py [--pairs 16 64] [--points 4096 12288] [--radii 3 7] [--rounds 5] [--seconds 1.0] [--out FILE]

min(n + 1, 64) 1920x1080 gray frames on a pan of (6, 2) px per frame over a smooth texture; pair k is (frame j, frame j + 1)
with j = k modulo the number of frames less one (at 64 pairs the last pair repeats the first: a call takes 64 frames); the
points are a lattice of the asked size. Arms, each captured into a HIP graph once and replayed, alternated round by round
in one process on one stream:
  pyramid          the pyramid call on the frames, levels = 4 (reads 4 B and writes 5.33 B per pixel)
  ingest           the identity-mode ingest launch on as many BGRA frames (reads 4 B, writes 4 B per pixel): the yardstick
  track_P_rR       the tracker on n pairs of P points at radius R, levels 4, 10 iterations, no gates, 16 lanes per point
  track_P_rR_l8    the same with 8 lanes per point (nm_klt_set_lanes; the setting is read when the call is captured)
  track_P_rR_l32   the same with 32 lanes per point
  track_P_rR_fb    the same with the forward-backward check (fb_max = 1)
  match_P          nm_sift_match_batch_dev_f32 on n pairs of P x P random unit descriptors, MATCH_MAX_BATCH pairs a call
One pair of every tracker arm is checked against the host twin before timing. Each arm is timed with device events after a
warm-up; a round replays an arm enough times for --seconds / --rounds of work. Prints one JSON line per (pairs, points)
and appends it to --out (default profiles/kklt_mi355x.jsonl): the median and min / max per arm over the rounds.
"""
import argparse
import os

import numpy as np

import karms
import torch

import niftymatch_amd as nm

FW, FH, LEVELS = 1920, 1080, 4


def make_frames(n, dev):
    g = torch.Generator(device="cpu").manual_seed(5)
    W, H = FW + 6 * n + 8, FH + 2 * n + 8
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                          indexing="ij")
    t = torch.zeros((H, W), device=dev)
    for _ in range(12):
        fx, fy, ph, amp = (float(v) for v in torch.rand(4, generator=g))
        t += (0.3 + 0.7 * amp) * torch.sin((fx - 0.5) * 0.7 * x + (fy - 0.5) * 0.7 * y + 6.28 * ph)
    t = 20 + 210 * (t - t.min()) / (t.max() - t.min())
    return [t[2 * k:2 * k + FH, 6 * k:6 * k + FW].contiguous() for k in range(n + 1)]


def lattice(points):
    step = int(np.sqrt(FW * FH / points))
    while True:
        xs, ys = nm.klt_grid_points(FW, FH, step)
        if len(xs) >= points:
            return xs[:points], ys[:points]
        step -= 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--points", type=int, nargs="+", default=[4096, 12288])
    ap.add_argument("--radii", type=int, nargs="+", default=[3, 7])
    karms.timing_args(ap, rounds=5, warmup=2, seconds=1.0, out=os.path.join(karms.ROOT, "profiles", "kklt_mi355x.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kklt.py measures on a GPU"
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    for n in a.pairs:
        nf = min(n + 1, nm.KLT_MAX_BATCH)
        grays = make_frames(nf - 1, dev)
        ia = [k % (nf - 1) for k in range(n)]
        bgra = [torch.stack([g, g, g, torch.full_like(g, 255)], -1).to(torch.uint8) for g in grays]
        pyrs, _ = nm.gray_pyramid_batch(grays, levels=LEVELS)
        for points in a.points:
            xs, ys = lattice(points)
            d_xs, d_ys = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
            d_n = torch.tensor([points], dtype=torch.int32, device=dev)
            desc = torch.nn.functional.normalize(torch.rand((nf, points, 128), device=dev), dim=2)
            results = [torch.empty(points, dtype=torch.int32, device=dev) for _ in range(n)]
            mb = nm.MATCH_MAX_BATCH
            ws = nm.MatchBatchDevWorkspace(min(n, mb), points, points, dev)
            outs, arms = {}, {}
            arms["pyramid"] = lambda: nm.gray_pyramid_batch(grays, levels=LEVELS, pyrs=pyrs)
            arms["ingest"] = lambda: nm.ingest_batch(bgra)

            def track(r, fb, name, lanes=0):
                nm.klt_set_lanes(lanes)
                outs[name] = nm.klt_track_batch_dev([pyrs[j] for j in ia], [pyrs[j + 1] for j in ia], FW, FH, [d_xs] * n, [d_ys] * n,
                                                    [d_n] * n, levels=LEVELS, radius=r, iterations=10, fb_max=fb, out=outs.get(name))
                nm.klt_set_lanes(0)
                return outs[name]

            def match():
                for k0 in range(0, n, mb):
                    k1 = min(n, k0 + mb)
                    nm.sift_match_batch_dev([desc[j] for j in ia[k0:k1]], [d_n] * (k1 - k0), [desc[j + 1] for j in ia[k0:k1]],
                                            [d_n] * (k1 - k0), results[k0:k1], workspace=ws)

            for r in a.radii:
                for fb in (0.0, 1.0):
                    name = "track_%d_r%d%s" % (points, r, "_fb" if fb else "")
                    arms[name] = lambda r=r, fb=fb, name=name: track(r, fb, name)
                for lanes in (8, 32):
                    name = "track_%d_r%d_l%d" % (points, r, lanes)
                    arms[name] = lambda r=r, name=name, lanes=lanes: track(r, 0.0, name, lanes)
            arms["match_%d" % points] = match
            with torch.cuda.stream(stream):
                torch.cuda.synchronize()
                for fn in arms.values():
                    fn()
                stream.synchronize()
                hp, _ = nm.gray_pyramid_host([grays[0].cpu().numpy(), grays[1].cpu().numpy()], levels=LEVELS)
                tracked = {}
                for name, o in outs.items():                        # pair 0 of every tracker arm against the host twin
                    r, fb = int(name.split("_r")[1].split("_")[0]), 1.0 if name.endswith("_fb") else 0.0
                    h = nm.klt_track_host([hp[0]], [hp[1]], FW, FH, [xs], [ys], [points], levels=LEVELS, radius=r, iterations=10,
                                          fb_max=fb)
                    assert np.array_equal(o.dst_xs[0].cpu().numpy().view(np.uint32), h.dst_xs[0].view(np.uint32)), name
                    assert int(o.count[0]) == int(h.count[0])
                    tracked[name] = float(o.count.sum()) / (n * points)
            graphs, kept = karms.capture(arms, stream)
            reps, times = karms.time_replays(graphs, stream, a.rounds, a.seconds, a.warmup)
            karms.emit({"tool": "kklt", "pairs": n, "frames": nf, "points": points, "frame": [FW, FH], "levels": LEVELS,
                        "rounds": a.rounds, "reps_per_round": reps, **karms.spread(times), "tracked_share": tracked}, a.out)
            del graphs, kept


if __name__ == "__main__":
    main()
