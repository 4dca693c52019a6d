"""The measuring loops of the stage tools (tools/k<stage>.py): a tool describes its arms, this module times them.

An arm is a name and a callable that issues the arm's work on the current stream. Two methods:
  eager    time_eager: warmup + rounds passes over the arms, one call of each per pass, each call between a pair of device
           events followed by a synchronise on the second; the passes after the warm-up are kept.
  replay   capture, then time_replays: every arm runs once eagerly and is captured into a HIP graph; every graph is replayed
           `warmup` times, probed once (one timed replay) to set reps = max(1, round(seconds / rounds / t_probe)), and then
           timed over `rounds` passes, `reps` replays of an arm between one event pair per pass.
In both the arms alternate inside every pass, in one process on one stream, and a tool reports the median and the min / max
over the kept passes (spread) as one JSON line (emit). Importing this module puts the repository root on sys.path, so that a
tool run from tools/ starts with `import karms` and finds niftymatch_amd after it.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def timing_args(ap, rounds, warmup, seconds=None, trace=False, out=None):
    """The timing arguments of a tool, with the tool's own defaults: --rounds and --warmup always, --seconds for the replay
    method, --trace and --out where the tool has them."""
    ap.add_argument("--rounds", type=int, default=rounds)
    ap.add_argument("--warmup", type=int, default=warmup)
    if seconds is not None:
        ap.add_argument("--seconds", type=float, default=seconds, help="work per arm, over all rounds")
    if trace:
        ap.add_argument("--trace", action="store_true")
    if out is not None:
        ap.add_argument("--out", default=out)


def event_timer(stream):
    """timer(fn, reps): microseconds per call of `reps` calls of fn between one pair of device events on `stream`."""
    def timer(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    return timer


def time_eager(runs, stream, rounds, warmup, timer=None):
    """times[arm] = the microseconds of the arm's call in each of the last `rounds` of warmup + rounds passes."""
    timer = timer or event_timer(stream)
    times = {name: [] for name in runs}
    with torch.cuda.stream(stream):
        for r in range(warmup + rounds):
            for name, fn in runs.items():
                t = timer(fn, 1)
                if r >= warmup:
                    times[name].append(t)
    return times


def capture(arms, stream):
    """(graphs, kept): every arm run once eagerly on `stream` (which loads its kernels), the device synchronised, then every
    arm captured into a graph of its own. kept[arm] is what the captured call returned: a graph writes into those tensors
    at every replay, so they live as long as the graph does."""
    with torch.cuda.stream(stream):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    graphs, kept = {}, {}
    for name, fn in arms.items():
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name], stream=stream):
            kept[name] = fn()
    return graphs, kept


def time_replays(replayables, stream, rounds, seconds, warmup, timer=None):
    """(reps, times) of graphs (anything with .replay()) or callables: `warmup` passes of one replay each, one timed replay
    of each to set reps[arm], then `rounds` passes of reps[arm] replays; times[arm] holds the microseconds per replay."""
    timer = timer or event_timer(stream)
    runs = {name: getattr(r, "replay", r) for name, r in replayables.items()}
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            for fn in runs.values():
                fn()
        reps = {name: max(1, int(round(seconds / rounds / (timer(fn, 1) * 1e-6)))) for name, fn in runs.items()}
        times = {name: [] for name in runs}
        for _ in range(rounds):
            for name, fn in runs.items():
                times[name].append(timer(fn, reps[name]))
    return reps, times


def spread(times):
    """The two entries every tool prints: the median and [min, max] of each arm's times."""
    return {"median_us": {k: float(np.median(t)) for k, t in times.items()},
            "min_max_us": {k: [float(min(t)), float(max(t))] for k, t in times.items()}}


def emit(record, out=None):
    """Prints the record as one JSON line and, with `out`, appends the line to that file (its folder is created)."""
    line = json.dumps(record)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")
