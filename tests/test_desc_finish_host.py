"""The descriptor finish through its host twin (nm_sift_desc_finish_host: the kernel's functions compiled for the host)
against the float64 restatement tests/desc_finish_ref.py. No GPU. The bound is derived in that module's docstring from
the operation count; the share of u8 codes that may differ by 1 (the model's 512 v within the bound of a half-integer) is
capped at 1 % and asserted on the model alone.
"""
import ctypes as C
import os

import numpy as np
import pytest

import desc_finish_ref as R

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [R.L2, R.ROOT]


def golden_rows():
    z = np.load(os.path.join(ROOT_DIR, "tests", "golden", "f160x120.npz"))
    return np.concatenate([z["desc0"], z["desc1"]]).astype(np.float32)


def random_rows(seed=3, n=400):
    """Non-negative rows of several kinds: uniform, sparse with a few dominant bins (the clip matters), scaled far up and down."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 1, (n, 128))
    a[n // 4: n // 2] *= rng.uniform(0, 1, (n // 4, 128)) < 0.15
    a[n // 2: 3 * n // 4] **= 6
    a *= 10.0 ** rng.integers(-12, 12, (n, 1))
    return a.astype(np.float32)


def edge_rows():
    e = np.zeros((8, 128), np.float32)
    e[1, 37] = 3.5                                   # one-hot
    e[2] = 0.75                                      # all equal
    e[3, 5:21] = np.linspace(1.0, 1.2, 16)           # every non-zero element above the clip after the first normalisation
    e[4] = 1.0
    e[4, 9] = np.inf                                 # an inf element: the sum is not finite
    e[5] = np.linspace(0.8e-30, 1.2e-30, 128)        # every square underflows: the sum is zero in binary32
    e[6] = np.linspace(0.8e-15, 1.2e-15, 128)        # small, squares still normal
    e[7] = 3.0e19                                    # squares overflow binary32: the sum is +inf
    return e                                         # row 0: all zero


def host(nm, rows, mode, **kw):
    f, u = nm.desc_finish_host([rows], [len(rows)], mode=mode, **kw)
    return (None if f is None else f[0]), (None if u is None else u[0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["golden", "random", "edge"])
def test_host_twin_within_the_derived_bound(nm, kind, mode):
    rows = {"golden": golden_rows, "random": random_rows, "edge": edge_rows}[kind]()
    f, u = host(nm, rows, mode)
    share = R.check(f, u, rows, mode)
    near = R.near_half(R.model(rows, mode)[0], mode)
    print("%s rows, mode %d: %d rows, excepted share %.2e" % (kind, mode, len(rows), share))
    assert near.mean() <= 0.01, "the inputs put too many codes next to a half-integer for the comparison to mean anything"
    if kind == "golden":                              # the clip is at work on real descriptors
        first = rows / np.sqrt((rows.astype(np.float64) ** 2).sum(1))[:, None]
        assert (first.max(1) > 0.2).mean() > 0.3 and len(rows) > 200
    if kind == "edge":
        live = R.model(rows, mode)[1]
        assert live.tolist() == [False, True, True, True, False, False, True, False]
        assert (u[1] == np.where(np.arange(128) == 37, 255, 0)).all()            # one-hot: 512 saturates
        assert (f[[0, 4, 5, 7]].view(np.uint32) == 0).all() and (u[[0, 4, 5, 7]] == 0).all()
        assert len(set(u[2].tolist())) == 1 and u[2][0] == 45            # 512 / sqrt(128) = 45.25 in both modes
        assert (u[3][5:21] > 120).all() and (u[3][:5] == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_output_sets_and_aliasing_agree(nm, mode):
    rows = np.concatenate([golden_rows()[:100], edge_rows()])
    f, u = host(nm, rows, mode)
    f_only, none = host(nm, rows, mode, want_u8=False)
    none2, u_only = host(nm, rows, mode, want_f32=False)
    fa, ua = host(nm, rows, mode, in_place=True)
    assert none is None and none2 is None
    for g in (f_only, fa):
        assert np.array_equal(g.view(np.uint32), f.view(np.uint32))
    for g in (u_only, ua):
        assert np.array_equal(g, u)


def test_counts_are_clipped_and_rows_beyond_them_untouched(nm):
    rows = golden_rows()[:64]
    lib = nm.lib()
    full_f, full_u = host(nm, rows, R.L2)
    for count, cap in ((0, 64), (-3, 64), (1, 64), (63, 64), (64, 64), (1000, 64), (40, 50), (70, 50)):
        src = [np.ascontiguousarray(rows), np.ascontiguousarray(rows[::-1])]
        f = np.full((2, 64, 128), 7.0, np.float32)
        u = np.full((2, 64, 128), 7, np.uint8)
        cnt = np.array([count, 5], np.int32)
        tab = lambda arrs: (C.c_void_p * 2)(*[a.ctypes.data for a in arrs])
        assert lib.nm_sift_desc_finish_host(2, tab(src), tab([cnt[0:1], cnt[1:2]]), cap, tab(list(f)), tab(list(u)), R.L2) == 0
        k = min(max(count, 0), cap)
        assert np.array_equal(f[0, :k].view(np.uint32), full_f[:k].view(np.uint32)) and np.array_equal(u[0, :k], full_u[:k])
        assert (f[0, k:] == 7.0).all() and (u[0, k:] == 7).all() and (f[1, 5:] == 7.0).all() and (u[1, 5:] == 7).all()
        assert np.array_equal(u[1, :5], full_u[::-1][:5])          # a frame's result does not depend on its slot


@pytest.mark.parametrize("mutant", [dict(clip=False), dict(renorm=False), dict(truncate=True)])
def test_the_checks_reject_mutants_of_the_model(nm, mutant):
    """A model without the clip, without the second normalisation, or truncating instead of rounding is NOT what the
    host twin computes: the same checks that pass against the model must fail against each of them. One exception is a
    fact of the mathematics, not a weakness of the checks: RootSIFT's L1 normalisation cancels any scale, so under
    NM_DESC_ROOT the second L2 normalisation changes nothing a real-number model could show."""
    rows = np.concatenate([golden_rows(), edge_rows()])
    for mode in MODES:
        f, u = host(nm, rows, mode)
        R.check(f, u, rows, mode)
        if mode == R.ROOT and mutant == dict(renorm=False):
            R.check(f, u, rows, mode, **mutant)
            continue
        with pytest.raises(AssertionError):
            R.check(f, u, rows, mode, **mutant)


def test_refusals(nm):
    lib = nm.lib()
    d = np.ones((8, 128), np.float32)
    f = np.full((2, 8, 128), 7.0, np.float32)
    u = np.full((2, 8, 128), 7, np.uint8)
    cnt = np.array([8], np.int32)
    tab = lambda a, k=2: (C.c_void_p * 64)(*([a.ctypes.data] * k))
    rows = lambda a, k=2: (C.c_void_p * 64)(*[a[i].ctypes.data for i in range(k)])

    def call(fn, n=2, cap=8, mode=0, **kw):
        a = dict(desc=tab(d), num=tab(cnt), f=rows(f), u=rows(u))
        a.update(kw)
        args = [n, a["desc"], a["num"], cap, a["f"], a["u"], mode]
        return fn(*(args + ([None] if fn is lib.nm_sift_desc_finish_batch_dev else [])))

    assert call(lib.nm_sift_desc_finish_host) == 0 and (u == 45).all()
    assert call(lib.nm_sift_desc_finish_host, f=None) == 0 and call(lib.nm_sift_desc_finish_host, u=None, mode=1) == 0
    f[:], u[:] = 7.0, 7
    bad = [dict(n=0), dict(n=-1), dict(n=65), dict(cap=0), dict(cap=-5), dict(cap=1 << 22), dict(mode=2), dict(mode=-1),
           dict(desc=None), dict(num=None), dict(f=None, u=None), dict(desc=tab(d, 1)), dict(num=tab(cnt, 1)),
           dict(f=rows(f, 1)), dict(u=rows(u, 1))]
    for fn in (lib.nm_sift_desc_finish_host, lib.nm_sift_desc_finish_batch_dev):      # both refuse before touching memory
        for kw in bad:
            assert call(fn, **kw) != 0, (fn.__name__, kw)
    assert (f == 7.0).all() and (u == 7).all()
    for name in ("nm_sift_desc_finish_batch_dev", "nm_sift_desc_finish_host"):
        assert name in nm.ABI_SYMBOLS
    assert nm.DESC_FINISH_MAX_BATCH == 64 and (nm.DESC_L2, nm.DESC_ROOT) == (0, 1)
    for kw in (dict(mode=2), dict(mode="l1"), dict(want_f32=False, want_u8=False), dict(capacity=9), dict(capacity=0)):
        with pytest.raises(nm.NmError):
            nm.desc_finish_host([d], [8], **kw)
    with pytest.raises(nm.NmError):
        nm.desc_finish_host([d] * 65, [8] * 65)
    with pytest.raises(nm.NmError):
        nm.desc_finish_host([np.ones((8, 64), np.float32)], [8])
    import torch
    with pytest.raises(nm.NmError):                   # the device wrapper wants device tensors
        nm.desc_finish_batch_dev([torch.zeros(8, 128)], [torch.zeros(1, dtype=torch.int32)], out_u8=True)
