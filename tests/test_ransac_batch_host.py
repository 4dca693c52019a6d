"""Host-side contract of the batched, device-sampled RANSAC (nm_ransac_batch_dev_f32): the sampler equals its numpy
restatement (include/nm_abi.h), the workspace bound grows with every dimension, and every invalid argument is refused
before any device access (so these run without a GPU)."""
import ctypes as C

import numpy as np
import pytest

M64 = (1 << 64) - 1


def splitmix64(c):
    """The standard SplitMix64 output function on state c (Python ints, wrapped to 64 bits)."""
    z = (c + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_py(seed, t, s, S, m):
    z = splitmix64(((seed & 0xFFFFFFFF) << 32) | ((t * S + s) & 0xFFFFFFFF))
    return ((z >> 32) * m) >> 32


def sample_np(seed, t, s, S, m):
    """Vectorised numpy restatement (uint64 arithmetic wraps, as the device's): arrays of t, s, m."""
    t, s, m = (np.asarray(v, np.uint64) for v in (t, s, m))
    with np.errstate(over="ignore"):
        z = (np.uint64(seed) << np.uint64(32)) | ((t * np.uint64(S) + s) & np.uint64(0xFFFFFFFF))
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return (((z >> np.uint64(32)) * m) >> np.uint64(32)).astype(np.int64)


def test_splitmix64_and_issue_vectors(nm):
    assert splitmix64(0) == 0xE220A8397B1DCDAF
    assert sample_py(0, 0, 0, 4, 1000) == 883
    assert sample_py(1, 0, 0, 4, 1000) == 766
    assert sample_py(0xFFFFFFFF, 4095, 1, 2, 12000) == 8043
    lib = nm.lib()
    assert lib.nm_ransac_batch_sample(0, 0, 0, 4, 1000) == 883
    assert lib.nm_ransac_batch_sample(1, 0, 0, 4, 1000) == 766
    assert lib.nm_ransac_batch_sample(0xFFFFFFFF, 4095, 1, 2, 12000) == 8043
    assert nm.ransac_batch_sample(0xFFFFFFFF, 4095, 1, 2, 12000) == 8043


def test_sampler_equals_numpy_restatement(nm):
    lib = nm.lib()
    rng = np.random.default_rng(11)
    for seed in (0, 1, 7, 0x12345678, 0xFFFFFFFF):
        for S in (1, 2, 4):
            t = rng.integers(0, 1 << 20, 300)
            t[:3] = [0, 1, (1 << 20) - 1]
            s = rng.integers(0, S, 300)
            m = rng.integers(1, 1 << 22, 300)
            m[:4] = [1, 2, 3, 12000]
            want = sample_np(seed, t, s, S, m)
            got = np.array([lib.nm_ransac_batch_sample(seed, int(a), int(b), S, int(c)) for a, b, c in zip(t, s, m)])
            assert np.array_equal(got, want), (seed, S)
            assert all(sample_py(seed, int(a), int(b), S, int(c)) == w for a, b, c, w in zip(t[:20], s[:20], m[:20], want[:20]))
    assert all(lib.nm_ransac_batch_sample(seed, t, 0, 4, 1) == 0 for seed in (0, 5, 0xFFFFFFFF) for t in range(50))
    # roughly uniform over [0, m)
    draws = sample_np(3, np.arange(40000), np.zeros(40000, np.int64), 1, np.full(40000, 10))
    assert set(np.unique(draws)) == set(range(10)) and np.bincount(draws).min() > 3700


def test_sampler_rejects_bad_arguments(nm):
    lib = nm.lib()
    for args in ((0, 0, 0, 3, 10), (0, 0, 0, 0, 10), (0, 0, 4, 4, 10), (0, 0, -1, 2, 10), (0, -1, 0, 1, 10),
                 (0, 1 << 20, 0, 1, 10), (0, 0, 0, 1, 0), (0, 0, 0, 1, -5)):
        assert lib.nm_ransac_batch_sample(*args) == -1, args


def test_workspace_bytes_positive_and_growing(nm):
    f = nm.lib().nm_ransac_batch_dev_workspace_bytes
    base = f(4, 1000, 512)
    assert base > 0
    assert f(5, 1000, 512) > base and f(4, 1001 + 255, 512) > base and f(4, 1000, 512 + 64) > base
    assert f(64, (1 << 22) - 1, 1 << 20) > f(64, 1 << 20, 1 << 20) > 0
    assert f(1, 1, 1) > 0
    # every pair's compacted points (16 B) and hypotheses (36 B) fit
    assert f(16, 12000, 4096) >= 16 * (12000 * 16 + 4096 * 36)
    for bad in ((0, 10, 10), (65, 10, 10), (1, 0, 10), (1, 1 << 22, 10), (1, 10, 0), (1, 10, (1 << 20) + 1)):
        assert f(*bad) == 0, bad
    assert nm.RANSAC_MAX_BATCH == 64 and nm.RANSAC_MAX_ITERATIONS == 1 << 20


INVALID_CASES = [
    dict(model=-1), dict(model=3), dict(n=0), dict(n=65), dict(n=-2), dict(iterations=0),
    dict(iterations=(1 << 20) + 1), dict(capA=0), dict(capA=1 << 22), dict(capA=-7), dict(thr=float("nan")),
    dict(thr=float("inf")), dict(thr=float("-inf")),
] + [dict(null=p) for p in ("src_x", "src_y", "d_nA", "dst_x", "dst_y", "matches", "seeds", "H_best", "best",
                            "position", "status", "workspace")] \
  + [dict(null_elem=p) for p in ("src_x", "src_y", "d_nA", "dst_x", "dst_y", "matches")]
HIP_ERROR_INVALID_VALUE = 1


def _call(nm, n=2, model=2, capA=100, iterations=64, thr=4.0, null=None, null_elem=None):
    """nm_ransac_batch_dev_f32 with exactly one invalid argument and FAKE device addresses for the others: the entry must
    return before it touches any of them. Only ever run by _child_main, in a process that sees no GPU."""
    fake = 0x1000
    nn = max(n, 1)
    ptrs = {}
    for name in ("src_x", "src_y", "d_nA", "dst_x", "dst_y", "matches"):
        vals = [fake] * nn
        if null_elem == name:
            vals[nn - 1] = None
        ptrs[name] = (C.c_void_p * nn)(*vals)
    seeds = (C.c_uint * nn)(*range(nn))
    args = dict(src_x=ptrs["src_x"], src_y=ptrs["src_y"], d_nA=ptrs["d_nA"], dst_x=ptrs["dst_x"], dst_y=ptrs["dst_y"],
                matches=ptrs["matches"], seeds=seeds, H_best=fake, best=fake, position=fake, status=fake,
                workspace=fake)
    if null is not None:
        args[null] = None
    return nm.lib().nm_ransac_batch_dev_f32(model, n, args["src_x"], args["src_y"], args["d_nA"], capA, args["dst_x"],
                                            args["dst_y"], args["matches"], iterations, thr, args["seeds"],
                                            args["H_best"], args["best"], args["position"], args["status"], None, None,
                                            args["workspace"], None)


def _child_main():
    """Runs every invalid case and prints the statuses as JSON. Refuses (exit 3, no call made) if a GPU is visible."""
    import json
    import sys
    import torch
    if torch.cuda.device_count() != 0:
        sys.exit(3)
    import niftymatch_amd as nm
    print(json.dumps([_call(nm, **kw) for kw in INVALID_CASES]))


@pytest.fixture(scope="module")
def invalid_statuses():
    """The invalid calls run in a fresh child process with every GPU hidden, so that even an entry whose checks had
    regressed could only fail to launch (hipErrorNoDevice), never dereference the fake addresses on a real device."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    path = [here, os.path.dirname(here)] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",
               PYTHONPATH=os.pathsep.join(path))
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + ["-c", "import test_ransac_batch_host as t; t._child_main()"], env=env,
                       cwd=here, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(out) == len(INVALID_CASES)
    return out


@pytest.mark.parametrize("case", range(len(INVALID_CASES)), ids=lambda i: "-".join("%s=%s" % kv for kv in INVALID_CASES[i].items()))
def test_invalid_arguments_refused_without_device_access(invalid_statuses, case):
    """hipErrorInvalidValue exactly: any other status (no device, launch failure) means the call got past its checks."""
    assert invalid_statuses[case] == HIP_ERROR_INVALID_VALUE, INVALID_CASES[case]


def test_python_wrapper_validates_before_the_call(nm):
    import torch
    x = torch.zeros(8)
    with pytest.raises(nm.NmError):
        nm.ransac_batch_dev(2, [], [], [], [], [], [])
    with pytest.raises(nm.NmError):
        nm.ransac_batch_dev(2, [x], [x, x], [x], [x], [x], [x])
    with pytest.raises(nm.NmError):
        nm.ransac_batch_dev(3, [x], [x], [x], [x], [x], [x])
    with pytest.raises(nm.NmError):
        nm.ransac_batch_dev(2, [x], [x], [x], [x], [x], [x], iterations=0)
    with pytest.raises(nm.NmError):
        nm.ransac_batch_dev(2, [x], [x], [x], [x], [x], [x], seeds=[1, 2])
    with pytest.raises(nm.NmError):
        nm.ransac_batch_dev(2, [x], [x], [x], [x], [x], [x], capA=9)
    with pytest.raises(nm.NmError):                     # host tensors are refused, never copied or computed on the CPU
        nm.ransac_batch_dev(2, [x], [x], [x], [x], [x], [x])
