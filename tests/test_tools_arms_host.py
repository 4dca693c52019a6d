"""tools/karms.py without a GPU: the order of the two measuring loops, pinned through the `timer` parameter, and the shape of
what spread and emit hand to a tool. A fake timer records (arm, reps) and returns a time chosen by the test; the arms record
every call made outside the timer (the warm-up replays). No stream is needed: the loops take stream=None here."""
import argparse
import importlib.util
import json
import os

import numpy as np

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "karms.py")
_spec = importlib.util.spec_from_file_location("karms", _PATH)
karms = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(karms)


class Call:
    """A callable arm that logs its direct calls."""

    def __init__(self, name, log):
        self.name, self.log = name, log

    def __call__(self):
        self.log.append(("run", self.name))


class Arm:
    """The same as a replayable: .replay() and no __call__, as a graph."""

    def __init__(self, name, log):
        self.name, self.log = name, log

    def replay(self):
        self.log.append(("run", self.name))


def fake_timer(log, us):
    """timer(fn, reps) that runs nothing, logs ("time", arm, reps) and returns us(arm, number of this call)."""
    def timer(fn, reps):
        name = getattr(fn, "__self__", fn).name
        log.append(("time", name, reps))
        return us(name, sum(1 for e in log if e[0] == "time") - 1)
    return timer


def test_time_eager_calls_every_arm_once_per_pass_and_keeps_the_last_rounds():
    log = []
    runs = {k: Call(k, log) for k in "abc"}
    times = karms.time_eager(runs, None, rounds=4, warmup=2, timer=fake_timer(log, lambda name, i: float(i)))
    assert log == [("time", k, 1) for _ in range(6) for k in "abc"]                  # 3 x 6 calls, arm order in each pass
    assert times == {k: [float(3 * p + j) for p in range(2, 6)] for j, k in enumerate("abc")}     # passes 2..5 of 0..5


def test_time_replays_warms_up_probes_sets_reps_and_alternates():
    log = []
    us = {"a": 10.0, "b": 1000.0, "c": 5e6}
    arms = {"a": Arm("a", log), "b": Arm("b", log), "c": Call("c", log)}                # graphs and a callable alike
    reps, times = karms.time_replays(arms, None, rounds=5, seconds=0.1, warmup=2, timer=fake_timer(log, lambda name, i: us[name]))
    assert reps == {k: max(1, int(round(0.1 / 5 / (t * 1e-6)))) for k, t in us.items()} == {"a": 2000, "b": 20, "c": 1}
    want = [("run", k) for _ in range(2) for k in "abc"]                                # warm-up: single replays, alternating
    want += [("time", k, 1) for k in "abc"]                                             # one probe of each
    want += [("time", k, reps[k]) for _ in range(5) for k in "abc"]                     # a b c, a b c, ... at each arm's reps
    assert log == want
    assert times == {k: [t] * 5 for k, t in us.items()}


def test_spread_is_median_and_min_max_as_plain_floats():
    s = karms.spread({"odd": [3.0, 1.0, 2.0], "even": [np.float64(4.0), 1.0, 3.0, 2.0]})
    assert s == {"median_us": {"odd": 2.0, "even": 2.5}, "min_max_us": {"odd": [1.0, 3.0], "even": [1.0, 4.0]}}
    assert list(s) == ["median_us", "min_max_us"]
    for k in ("odd", "even"):
        assert type(s["median_us"][k]) is float and all(type(v) is float for v in s["min_max_us"][k])
    assert json.loads(json.dumps(s)) == s


def test_emit_prints_one_line_and_appends_to_a_new_folder(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rec = {"tool": "t", "median_us": {"a": 1.5}}
    karms.emit(rec)
    assert capsys.readouterr().out == json.dumps(rec) + "\n"
    assert list(tmp_path.iterdir()) == []                                               # no file without `out`
    out = tmp_path / "deeper" / "still" / "t.jsonl"
    karms.emit(rec, str(out))
    karms.emit({"tool": "u"}, str(out))
    assert capsys.readouterr().out.count("\n") == 2
    assert [json.loads(l) for l in out.read_text().splitlines()] == [rec, {"tool": "u"}]


def test_timing_args_adds_what_the_tool_has_with_its_defaults():
    ap = argparse.ArgumentParser()
    karms.timing_args(ap, rounds=12, warmup=2, trace=True)
    a = ap.parse_args([])
    assert vars(a) == {"rounds": 12, "warmup": 2, "trace": False}
    ap = argparse.ArgumentParser()
    karms.timing_args(ap, rounds=5, warmup=2, seconds=1.0, out="x.jsonl")
    assert vars(ap.parse_args([])) == {"rounds": 5, "warmup": 2, "seconds": 1.0, "out": "x.jsonl"}
    assert vars(ap.parse_args("--rounds 2 --seconds 0.05 --warmup 1 --out y".split())) == \
        {"rounds": 2, "warmup": 1, "seconds": 0.05, "out": "y"}
