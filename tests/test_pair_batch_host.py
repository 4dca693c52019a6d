"""The pair-batch convention itself (csrc/nm_pair_batch.hpp and the marshalling helpers of niftymatch_amd/__init__.py), through
the three host twins and the seven public wrappers. No GPU: the twins run the check the device entries run, and the device
wrappers are given host tensors, which they refuse only after every check that this file is about.
"""
import ctypes as C

import numpy as np
import pytest

INVALID = 1                                      # hipErrorInvalidValue
N, CAP, SLOTS = 2, 4, 3                          # pairs, capacity, table length: slot 2 is unused


class _Call:
    """One valid call of a host twin with n = 2 pairs of capacity 4 and tables 3 long; run() applies overrides by name."""

    def __init__(self, lib, twin, slots=SLOTS):
        self.keep = []
        desc = [self._a(np.zeros((CAP, 128), np.float32)) for _ in range(slots)]
        xy = [self._a(np.arange(CAP, dtype=np.float32)) for _ in range(slots)]
        size = [self._a(np.array([CAP], np.int32)) for _ in range(slots)]
        mt = [self._a(np.arange(CAP, dtype=np.int32)) for _ in range(slots)]
        out_i = [self._a(np.zeros(CAP, np.int32)) for _ in range(slots)]
        out_f = [self._a(np.zeros(CAP, np.float32)) for _ in range(slots)]
        H = self._a(np.tile(np.eye(3, dtype=np.float32).reshape(-1), slots))
        vec = lambda dt: self._a(np.zeros(slots, dt)).ctypes.data
        tab = self.table
        if twin == "refit":
            self.fn = lib.nm_ransac_refit_host_f32
            self.args = [("model", 0), ("n", N), ("src_x", tab(xy)), ("src_y", tab(xy)), ("nA", tab(size)), ("capA", CAP),
                         ("dst_x", tab(xy)), ("dst_y", tab(xy)), ("matches", tab(mt)), ("H_in", H.ctypes.data), ("status_in", None),
                         ("thr", 4.0), ("rounds", 1), ("H_out", self._a(np.zeros(9 * slots, np.float32)).ctypes.data),
                         ("count", vec(np.int32)), ("status", vec(np.int32)), ("rounds_done", vec(np.int32)), ("mask", None),
                         ("rms", None)]
            self.required, self.optional = ["src_x", "src_y", "nA", "dst_x", "dst_y", "matches"], []
        elif twin == "guided":
            self.fn = lib.nm_sift_match_guided_host_f32
            self.args = [("n", N), ("A", tab(desc)), ("ax", tab(xy)), ("ay", tab(xy)), ("nA", tab(size)), ("capA", CAP),
                         ("B", tab(desc)), ("bx", tab(xy)), ("by", tab(xy)), ("nB", tab(size)), ("capB", CAP), ("H", H.ctypes.data),
                         ("status_in", None), ("radius2", 9.0), ("ambiguity", 0.8), ("max_distance", float("inf")),
                         ("result", tab(out_i)), ("count", vec(np.int32)), ("best_distance", tab(out_f))]
            self.required, self.optional = ["A", "ax", "ay", "nA", "B", "bx", "by", "nB", "result"], ["best_distance"]
        else:
            self.fn = lib.nm_sift_match_mutual_host_f32
            self.args = [("n", N), ("A", tab(desc)), ("nA", tab(size)), ("capA", CAP), ("B", tab(desc)), ("nB", tab(size)),
                         ("capB", CAP), ("matches", tab(mt)), ("result", tab(out_i)), ("count", vec(np.int32)),
                         ("forward_distance", tab(out_f))]
            self.required, self.optional = ["A", "nA", "B", "nB", "matches", "result"], ["forward_distance"]

    def _a(self, a):
        self.keep.append(a)
        return a

    def table(self, arrays):
        t = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
        self.keep.append(t)
        return t

    def without_slot(self, name, k):
        t = dict(self.args)[name]
        return (C.c_void_p * len(t))(*[None if i == k else t[i] for i in range(len(t))])

    def run(self, **over):
        assert all(k in dict(self.args) for k in over)
        return self.fn(*[over.get(k, v) for k, v in self.args])


@pytest.mark.parametrize("twin", ["refit", "guided", "mutual"])
def test_the_shared_predicates_through_the_host_twins(nm, twin):
    c = _Call(nm.lib(), twin)
    assert c.run() == 0
    for name in c.required + c.optional:
        assert c.run(**{name: c.without_slot(name, 1)}) == INVALID, (twin, name, "null in used slot 1")
        assert c.run(**{name: c.without_slot(name, 2)}) == 0, (twin, name, "null in unused slot 2")
    for name in c.required:
        assert c.run(**{name: None}) == INVALID, (twin, name, "required table missing")
    for name in c.optional:
        assert c.run(**{name: None}) == 0, (twin, name, "optional table missing")
    assert c.run(n=0) == INVALID and c.run(capA=0) == INVALID and c.run(capA=1 << 22) == INVALID
    assert _Call(nm.lib(), twin, slots=65).run(n=65) == INVALID        # 65 valid slots: the range alone refuses
    assert _Call(nm.lib(), twin, slots=64).run(n=64) == 0


def test_the_range_predicate_through_the_workspace_sizes(nm):
    lib = nm.lib()
    assert lib.nm_ransac_batch_dev_workspace_bytes(64, (1 << 22) - 1, 1) > 0
    assert lib.nm_sift_match_mutual_workspace_bytes(64, (1 << 22) - 1) > 0
    for n, cap in ((0, 4), (65, 4), (2, 0), (2, 1 << 22)):
        assert lib.nm_ransac_batch_dev_workspace_bytes(n, cap, 1) == 0 and lib.nm_sift_match_mutual_workspace_bytes(n, cap) == 0


# ---- the seven wrappers: per wrapper the per-pair lists in call order, and whether it takes H / status ----
POINTS = ("xy", "xy", "size", "xy", "xy", "matches")
WRAPPERS = {
    "ransac_batch_dev": (POINTS, False), "ransac_refit_batch_dev": (POINTS, True), "ransac_refit_host": (POINTS, True),
    "sift_match_guided_batch_dev": (("desc", "xy", "xy", "size", "desc", "xy", "xy", "size"), True),
    "sift_match_guided_host": (("desc", "xy", "xy", "size", "desc", "xy", "xy", "size"), True),
    "sift_match_mutual_batch_dev": (("desc", "size", "desc", "size", "matches"), False),
    "sift_match_mutual_host": (("desc", "size", "desc", "size", "matches"), False),
}


def _wrapper_args(name, n=N):
    import torch
    host = name.endswith("_host")
    make = {"desc": lambda: np.zeros((CAP, 128), np.float32), "xy": lambda: np.arange(CAP, dtype=np.float32),
            "matches": lambda: np.arange(CAP, dtype=np.int32), "size": lambda: np.array([CAP], np.int32)}
    conv = (lambda a: a) if host else torch.from_numpy
    kinds, has_H = WRAPPERS[name]
    lists = [[CAP if host and kind == "size" else conv(make[kind]()) for _ in range(n)] for kind in kinds]
    args = ([0] if name.startswith("ransac") else []) + lists                     # RANSAC and refit: the model first
    kw = dict(H=conv(np.tile(np.eye(3, dtype=np.float32).reshape(-1), n)), status=conv(np.ones(n, np.int32))) if has_H else {}
    return args, kw, len(args) - len(lists)


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_the_wrappers_share_their_refusals(nm, name):
    import torch
    fn = getattr(nm, name)
    args, kw, first = _wrapper_args(name)
    if name.endswith("_host"):
        fn(*args, **kw)                                                           # the arguments below are valid ...
    else:
        with pytest.raises(nm.NmError, match="current device"):                   # ... up to the device check
            fn(*args, **kw)
    short = list(args)
    short[first + 1] = short[first + 1][:-1]
    with pytest.raises(nm.NmError, match="lists of one length"):
        fn(*short, **kw)
    many, many_kw, _ = _wrapper_args(name, 65)
    with pytest.raises(nm.NmError, match="lists of one length"):
        fn(*many, **many_kw)
    with pytest.raises(nm.NmError, match="smaller than the capacity"):
        fn(*args, capA=CAP + 1, **kw)
    with pytest.raises(nm.NmError, match="capacity 0 outside"):
        fn(*args, capA=0, **kw)
    if "H" in kw:
        cut = lambda t, m: t[:m] if name.endswith("_host") else t[:m].clone()
        with pytest.raises(nm.NmError, match="H must hold"):
            fn(*args, **dict(kw, H=cut(kw["H"], 9 * N - 1)))
        longer = np.ones(N + 1, np.int32)
        with pytest.raises(nm.NmError, match="H must hold"):
            fn(*args, **dict(kw, status=longer if name.endswith("_host") else torch.from_numpy(longer)))
