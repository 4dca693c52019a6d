"""tools/karms.py on the device: the loops replay exactly what they report. Two arms that each add 1 to a tensor of their own,
so a tensor's value is the number of times its arm ran. Needs torch only, none of the library's kernels."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "karms.py")
_spec = importlib.util.spec_from_file_location("karms", _PATH)
karms = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(karms)

N = 65536


def test_replays_and_eager_calls_are_counted_exactly(cuda):
    import torch
    x, y = torch.zeros(N, device=cuda), torch.zeros(N, device=cuda)
    arms = {"a": lambda: x.add_(1), "b": lambda: y.add_(1)}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    warmup, rounds = 1, 2
    graphs, kept = karms.capture(arms, stream)
    reps, times = karms.time_replays(graphs, stream, rounds, 0.02, warmup)
    torch.cuda.synchronize()
    # capture: one eager run (the capture itself runs nothing); time_replays: `warmup` single replays, one probe replay,
    # then `rounds` passes of reps[arm] replays
    for t, k in ((x, "a"), (y, "b")):
        want = 1 + warmup + 1 + rounds * reps[k]
        assert reps[k] >= 1 and want < 2 ** 24                             # fp32 counts exactly up to there
        assert len(times[k]) == rounds and all(v > 0 for v in times[k])
        assert float(t.min()) == float(t.max()) == float(want), (k, reps[k])

    x.zero_()
    y.zero_()
    torch.cuda.synchronize()
    times = karms.time_eager(arms, stream, rounds=3, warmup=1)
    torch.cuda.synchronize()
    for t, k in ((x, "a"), (y, "b")):
        assert float(t.min()) == float(t.max()) == 4.0                     # warmup + rounds calls of each arm
        assert len(times[k]) == 3 and all(v > 0 for v in times[k])
    del graphs, kept
