"""The schedule of a detect/describe call (niftymatch_amd/csrc/nm_frame_plan.hpp; what it orchestrates: the reference's client
loop, sift/siftfunctions.cu:42-181) is data: nm_sift_frame_plan hands out the ops the frame driver walks -- launches, streams,
events -- for a resolved configuration. It is a host function, so everything the issue orders rely on is checked here without
a GPU, for every configuration: no two ops that touch the same memory are unordered, the plan can be captured, both helper
streams are joined on every error path, and the next call stands behind all of it.

Configurations the driver never resolves to (the octave tail or a split description with an order other than 0, the tail with
split != first_tail or with DoG planes, split >= octaves) are INVALID: the entry point returns 0 for them.

One thing the model below knows about and allows: the scan of octave o rewrites oct_base[o] with the value the scan of octave
o - 1 put there (it is the running total it has just read). An early description of the octaves [0, s) reads oct_base[s] while
the scan of octave s, unordered against it, stores that same value again. The rewrite is modelled as a read."""
import ctypes as C
import itertools

import pytest

BASE, LEV, DET, TAIL, TSCAN, DESCR, REC, WAIT, JOIN = range(9)
CALLER, SIDE, DESC = 0, 1, 2
NONE, PYR, TOP, EDET, EDESC, EJOIN = -1, 0, 1, 2, 3, 4
MAX_OPS = 160
LAUNCHES = {BASE: 1, DET: 3, TAIL: 1, TSCAN: 1, DESCR: 2, REC: 0, WAIT: 0, JOIN: 0}


def plan(nm, octaves, first_tail=None, split=0, dogs=0, order=0):
    buf = (C.c_int * (6 * MAX_OPS))()
    n = nm.lib().nm_sift_frame_plan(octaves, octaves if first_tail is None else first_tail, split, dogs, order, buf, MAX_OPS)
    assert 0 <= n <= MAX_OPS
    return [tuple(buf[6 * i: 6 * i + 6]) for i in range(n)]


# ---- frozen sequences: written out from the parent's driver, op for op -------------------------------------------------

def _z(kind, stream, octave=0, lo=0, hi=0, event=NONE):
    return (kind, stream, octave, lo, hi, event)


FROZEN = {
    "3 octaves, order 0": (dict(octaves=3), [
        _z(BASE, CALLER),
        _z(LEV, CALLER, 0, 1, 5), _z(REC, CALLER, 0, event=PYR), _z(WAIT, SIDE, 0, event=PYR), _z(DET, SIDE, 0),
        _z(LEV, CALLER, 1, 1, 5), _z(REC, CALLER, 1, event=PYR), _z(WAIT, SIDE, 1, event=PYR), _z(DET, SIDE, 1),
        _z(LEV, CALLER, 2, 1, 5), _z(REC, CALLER, 2, event=PYR), _z(WAIT, SIDE, 2, event=PYR), _z(DET, SIDE, 2),
        _z(DESCR, SIDE, 0, 0, 3),
        _z(JOIN, SIDE, event=EJOIN)]),
    "3 octaves, order 1": (dict(octaves=3, order=1), [
        _z(BASE, CALLER),
        _z(LEV, CALLER, 0, 1, 3), _z(REC, CALLER, 0, event=PYR), _z(WAIT, SIDE, 0, event=PYR), _z(LEV, SIDE, 0, 4, 5), _z(DET, SIDE, 0),
        _z(LEV, CALLER, 1, 1, 3), _z(REC, CALLER, 1, event=PYR), _z(WAIT, SIDE, 1, event=PYR), _z(LEV, SIDE, 1, 4, 5), _z(DET, SIDE, 1),
        _z(LEV, CALLER, 2, 1, 3), _z(REC, CALLER, 2, event=PYR), _z(WAIT, SIDE, 2, event=PYR), _z(LEV, SIDE, 2, 4, 5), _z(DET, SIDE, 2),
        _z(DESCR, SIDE, 0, 0, 3),
        _z(JOIN, SIDE, event=EJOIN)]),
    "3 octaves, order 2": (dict(octaves=3, order=2), [
        _z(BASE, CALLER),
        _z(LEV, CALLER, 0, 1, 3), _z(REC, CALLER, 0, event=PYR), _z(WAIT, DESC, 0, event=PYR), _z(LEV, DESC, 0, 4, 5),
        _z(REC, DESC, 0, event=TOP), _z(WAIT, SIDE, 0, event=TOP), _z(DET, SIDE, 0),
        _z(LEV, CALLER, 1, 1, 3), _z(REC, CALLER, 1, event=PYR), _z(WAIT, DESC, 1, event=PYR), _z(LEV, DESC, 1, 4, 5),
        _z(REC, DESC, 1, event=TOP), _z(WAIT, SIDE, 1, event=TOP), _z(DET, SIDE, 1),
        _z(LEV, CALLER, 2, 1, 3), _z(REC, CALLER, 2, event=PYR), _z(WAIT, DESC, 2, event=PYR), _z(LEV, DESC, 2, 4, 5),
        _z(REC, DESC, 2, event=TOP), _z(WAIT, SIDE, 2, event=TOP), _z(DET, SIDE, 2),
        _z(DESCR, SIDE, 0, 0, 3),
        _z(JOIN, DESC, event=EDESC), _z(JOIN, SIDE, event=EJOIN)]),
    "4 octaves, tail T = 2": (dict(octaves=4, first_tail=2, split=2), [
        _z(BASE, CALLER),
        _z(LEV, CALLER, 0, 1, 5), _z(REC, CALLER, 0, event=PYR), _z(WAIT, SIDE, 0, event=PYR), _z(DET, SIDE, 0),
        _z(LEV, CALLER, 1, 1, 5), _z(REC, CALLER, 1, event=PYR), _z(TAIL, CALLER, 2), _z(WAIT, SIDE, 1, event=PYR), _z(DET, SIDE, 1),
        _z(REC, SIDE, event=EDET), _z(DESCR, SIDE, 0, 0, 2),
        _z(WAIT, CALLER, event=EDET), _z(TSCAN, CALLER, 2), _z(DESCR, CALLER, 0, 2, 4),
        _z(JOIN, SIDE, event=EJOIN)]),
    "3 octaves, split 2, order 0": (dict(octaves=3, split=2), [
        _z(BASE, CALLER),
        _z(LEV, CALLER, 0, 1, 5), _z(REC, CALLER, 0, event=PYR), _z(WAIT, SIDE, 0, event=PYR), _z(DET, SIDE, 0),
        _z(LEV, CALLER, 1, 1, 5), _z(REC, CALLER, 1, event=PYR), _z(WAIT, SIDE, 1, event=PYR), _z(DET, SIDE, 1),
        _z(REC, SIDE, event=EDET), _z(WAIT, DESC, event=EDET), _z(DESCR, DESC, 0, 0, 2),
        _z(LEV, CALLER, 2, 1, 5), _z(REC, CALLER, 2, event=PYR), _z(WAIT, SIDE, 2, event=PYR), _z(DET, SIDE, 2),
        _z(DESCR, SIDE, 0, 2, 3),
        _z(JOIN, DESC, event=EDESC), _z(JOIN, SIDE, event=EJOIN)]),
}


@pytest.mark.parametrize("name", sorted(FROZEN))
def test_plan_is_the_parents_issue_sequence(nm, name):
    cfg, want = FROZEN[name]
    assert plan(nm, **cfg) == want


# ---- the kernels' contract, restated: what each op reads and writes -----------------------------------------------------

def _touches(op, octaves, first_tail, dogs):
    """(reads, writes) of an op. Planes: ("lev", o, i), ("dog", o, i), ("grad", o, p). Detection's staging, counts and offsets
    are one buffer set per call ("staging"); the tail stages per octave ("tstage", o). The book is oct_base[j] ("base", j),
    the rows of octave o ("lvl", o) and the running total with the caller's counter ("total"); the keypoint list and the
    outputs (descriptors, orientations, x / y) are octave-major slots ("kpts", o), ("out", o)."""
    kind, _, o, lo, hi, _ = op
    R, Wr = set(), set()
    if kind == BASE:
        Wr.add(("lev", 0, 0))
    elif kind == LEV:
        for i in range(lo, hi + 1):
            R.add(("lev", o, i - 1))
            if i < 5 or not dogs:                  # level 5 is stored only where detection reads the levels
                Wr.add(("lev", o, i))
            if dogs:
                Wr.add(("dog", o, i - 1))
            if 2 <= i <= 4:
                Wr.add(("grad", o, i - 2))
            if i == 3 and o + 1 < octaves:
                Wr.add(("lev", o + 1, 0))
    elif kind == DET:
        R |= {("dog", o, i) for i in range(5)} if dogs else {("lev", o, i) for i in range(6)}
        R |= {"staging", ("base", o)} | ({"total"} if o else set())
        Wr |= {"staging", "total", ("base", o + 1), ("lvl", o), ("kpts", o)}
        if o == 0:
            Wr.add(("base", 0))
    elif kind == TAIL:
        R.add(("lev", first_tail, 0))
        Wr.add("tstate")
        for t in range(first_tail, octaves):
            Wr |= {("lev", t, i) for i in range(1, 6)} | {("grad", t, p) for p in range(3)} | {("tstage", t)}
            if t + 1 < octaves:
                Wr.add(("lev", t + 1, 0))
    elif kind == TSCAN:
        R |= {"total", ("base", first_tail)} | {("tstage", t) for t in range(first_tail, octaves)}
        Wr.add("total")
        for t in range(first_tail, octaves):
            Wr |= {("base", t + 1), ("lvl", t), ("kpts", t)}
    elif kind == DESCR:
        R |= {("base", j) for j in range(lo, hi + 1)}
        for t in range(lo, hi):
            R |= {("grad", t, p) for p in range(3)} | {("kpts", t)}
            Wr.add(("out", t))
    return R, Wr


def _happens_before(ops):
    """reach[b] = bit set of the ops that happen before op b: stream order, RECORD -> WAIT, and a JOIN stands on its helper
    stream (the record) and on the caller's (the wait). A last node, the end of the caller's stream, is appended."""
    last = {}                                       # stream -> index of its latest op
    recorded = {}                                   # (event, octave) -> index of the latest record
    reach = []
    problems = []
    for k, (kind, stream, o, lo, hi, ev) in enumerate(ops):
        before = 0
        preds = [last.get(stream)]
        key = (ev, o if ev in (PYR, TOP) else 0)
        if kind == WAIT:
            if key not in recorded:
                problems.append("op %d waits for an event that no earlier op records" % k)
            preds.append(recorded.get(key))
        if kind == JOIN:
            preds.append(last.get(CALLER))
            last[CALLER] = k
        for p in preds:
            if p is not None:
                before |= reach[p] | (1 << p)
        reach.append(before)
        last[stream] = k
        if kind == REC:
            recorded[key] = k
    end = last.get(CALLER)
    reach.append(reach[end] | (1 << end))
    return reach, problems


def check(ops, octaves, first_tail, split, dogs):
    """Every property of a plan; returns the list of what is wrong with it."""
    reach, problems = _happens_before(ops)
    n = len(ops)
    touch = [_touches(op, octaves, first_tail, dogs) for op in ops]
    for a, b in itertools.combinations(range(n), 2):
        (Ra, Wa), (Rb, Wb) = touch[a], touch[b]
        clash = (Wa & (Rb | Wb)) | (Ra & Wb)
        if clash and not (reach[b] >> a) & 1:
            problems.append("ops %d %r and %d %r are unordered on %r" % (a, ops[a], b, ops[b], sorted(map(str, clash))[:3]))
    # the next call starts on the caller's stream: everything stands before its end
    if reach[n] != (1 << n) - 1:
        problems.append("ops %r are not ordered before the end of the caller's stream"
                        % [k for k in range(n) if not (reach[n] >> k) & 1])
    # joins: last, description stream before side stream, into the caller's stream only, one per helper that waited
    joins = [op[1] for op in ops if op[0] == JOIN]
    waited = {op[1] for op in ops if op[0] == WAIT} - {CALLER}
    if [op[0] for op in ops[n - len(joins):]] != [JOIN] * len(joins):
        problems.append("the JOIN ops are not the plan's last ops")
    if CALLER in joins or joins != sorted(set(joins), reverse=True) or set(joins) != waited:
        problems.append("joins %r for the helpers %r that waited" % (joins, sorted(waited)))
    # helpers that launch without having waited would run ahead of the caller's stream
    for k, op in enumerate(ops):
        if op[1] != CALLER and op[0] != WAIT and not any(p[0] == WAIT and p[1] == op[1] for p in ops[:k]):
            problems.append("op %d runs on a helper stream that has not waited for anything" % k)
    # fork tree: a helper forked from another helper (its first wait names that one's event) is never waited for by it
    where = {}
    parent = {}
    for kind, stream, o, lo, hi, ev in ops:
        key = (ev, o if ev in (PYR, TOP) else 0)
        if kind == REC:
            where[key] = stream
        if kind == WAIT and stream != CALLER and stream not in parent:
            parent[stream] = where.get(key)
    for kind, stream, o, lo, hi, ev in ops:
        key = (ev, o if ev in (PYR, TOP) else 0)
        if kind == WAIT and stream != CALLER and parent.get(where.get(key)) == stream:
            problems.append("stream %d waits for stream %d, which was forked from it" % (stream, where[key]))
    # launches: nm_sift_arena_launches_per_call's documented values
    launches = sum(op[4] - op[3] + 1 if op[0] == LEV else LAUNCHES[op[0]] for op in ops)
    want = 1 + 8 * first_tail + 2 + 4 if first_tail < octaves else 1 + 8 * octaves + 2 + (2 if split else 0)
    if launches != want:
        problems.append("%d launches, documented %d" % (launches, want))
    # the walker's error rule: op k fails -> nothing more is launched, the JOIN ops of every stream on which a WAIT was
    # issued successfully are still executed, description stream first
    for k in range(n):
        forked = {op[1] for op in ops[:k] if op[0] == WAIT} - {CALLER}
        executed = [op[1] for op in ops if op[0] == JOIN and op[1] in forked]
        if set(executed) != forked or executed != sorted(executed, reverse=True):
            problems.append("an error at op %d leaves the forked streams %r with the joins %r" % (k, sorted(forked), executed))
    return problems


def _valid(octaves, first_tail, split, dogs, order):
    if first_tail is not None and first_tail != octaves:       # first_tail == octaves says "no tail", as None does here
        return first_tail < octaves and split == first_tail and not dogs and order == 0
    return split < octaves and (split == 0 or order == 0)


@pytest.mark.parametrize("octaves", [1, 2, 3, 4, 5, 6, 7, 8, 20])
def test_every_configuration_is_hazard_free_capturable_and_joined(nm, octaves):
    seen = 0
    for order, first_tail, split, dogs in itertools.product((0, 1, 2), (None, 1, 2, 3), (0, 1, 2, 3), (0, 1)):
        ops = plan(nm, octaves, first_tail, split, dogs, order)
        assert bool(ops) == _valid(octaves, first_tail, split, dogs, order), (octaves, order, first_tail, split, dogs)
        if ops:
            seen += 1
            assert ops[0][0] == BASE and all(0 <= op[2] < octaves for op in ops)
            assert check(ops, octaves, octaves if first_tail is None else first_tail, split, dogs) == [], \
                (octaves, order, first_tail, split, dogs)
    assert seen >= 6                                # three orders, with and without DoG planes


def test_out_of_range_configurations_have_no_plan(nm):
    for cfg in (dict(octaves=0), dict(octaves=21), dict(octaves=3, order=3), dict(octaves=3, order=-1), dict(octaves=3, split=-1),
                dict(octaves=3, first_tail=0, split=0), dict(octaves=3, first_tail=4, split=4)):
        assert plan(nm, **cfg) == [], cfg
    assert len(plan(nm, 20, order=2)) == 1 + 7 * 20 + 1 + 2          # the widest per-octave plan fits the entry point's buffer


@pytest.mark.parametrize("name", sorted(FROZEN))
def test_the_checks_notice_a_missing_edge(nm, name):
    """Teeth: a plan with any ONE of its waits or records taken out is reported."""
    cfg, _ = FROZEN[name]
    ops = plan(nm, **cfg)
    octaves, first_tail = cfg["octaves"], cfg.get("first_tail", cfg["octaves"])
    assert check(ops, octaves, first_tail, cfg.get("split", 0), 0) == []
    edges = [k for k, op in enumerate(ops) if op[0] in (WAIT, REC)]
    assert len(edges) >= 6
    for k in edges:
        assert check(ops[:k] + ops[k + 1:], octaves, first_tail, cfg.get("split", 0), 0), "op %d %r is not needed?" % (k, ops[k])
