"""The one-item drop-in entry points against plain numpy. nm_downsample2_f32, nm_subtract_f32 and nm_compute_sift_descriptors are
the one-item case of their batched launchers; nm_compact_keypoints keeps kernels of its own beside nm_compact_keypoints3's and must
agree with them list for list. Sizes: where the kernels change path -- one element, either side of a 256-thread workgroup, two
counts per scan thread, the scan's non-register path, one past each grid cap -- with guard words behind every buffer written and
behind the exact workspace. (The orientation and descriptor entries are held by test_gpu_describe_float64.py.)"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD_BYTES = 4096
GUARD = 0xA5
FILL = 7.0


def _t(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _same_bits(got, ref, what):
    got = got.detach().cpu().numpy()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), "%s: %d of %d words differ" % (what, int(bad.sum()), bad.size)


@functools.lru_cache(maxsize=None)
def _dense_map(n, filling):
    """n float4 entries, shared between the tests and never modified; `filling`: 'none' valid, 'all' valid, 'some' = about 3 %
    valid at random with w >= 0 (0 included)"""
    rng = np.random.default_rng(1000 + n % 997 + {"none": 0, "all": 1, "some": 2}[filling])
    d = rng.random((n, 4), dtype=np.float32) * np.float32(1000.0)
    if filling == "none":
        d[:, 3] = -1.0
    elif filling == "all":
        d[:, 3] = rng.integers(0, 3, n).astype(np.float32)
    else:
        valid = rng.random(n) < 0.03
        d[:, 3] = np.where(valid, rng.integers(0, 3, n), -1).astype(np.float32)
    return d


def _workspace(nbytes, cuda):
    """exactly nbytes of workspace followed by GUARD_BYTES of guard pattern (the whole tensor starts as the pattern)"""
    import torch
    return torch.full((nbytes + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=cuda)


def _compact_single(nm, cuda, dense):
    """nm_compact_keypoints on a dense map (numpy, n x 4) -> (count, out tensor of n + 1 entries pre-filled with FILL)"""
    import torch
    n = dense.shape[0]
    lib = nm.lib()
    nbytes = lib.nm_compact_workspace_bytes(n)
    assert nbytes == 2 * ((n + 255) // 256) * 4
    ws = _workspace(nbytes, cuda)
    out = torch.full((n + 1, 4), FILL, dtype=torch.float32, device=cuda)
    cnt = torch.full((2,), -77, dtype=torch.int32, device=cuda)
    src = _t(dense, cuda)
    assert lib.nm_compact_keypoints(src.data_ptr(), n, out.data_ptr(), cnt.data_ptr(), ws.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == GUARD).all()), "the one-level compaction wrote behind its 2 * nb ints of workspace"
    assert int(cnt[1]) == -77, "more than one total was written"
    return int(cnt[0]), out


COMPACT_SIZES = [1, 255, 256, 257, 262145, 3145729]     # the last two: 1 025 and 12 289 workgroups of 256 entries


@pytest.mark.parametrize("filling", ["none", "all", "some"])
@pytest.mark.parametrize("n", COMPACT_SIZES)
def test_compaction_of_one_level(nm, cuda, n, filling):
    dense = _dense_map(n, filling)
    want = dense[dense[:, 3] >= 0]
    count, out = _compact_single(nm, cuda, dense)
    assert count == len(want)
    _same_bits(out[:count], want, "compacted list")
    assert bool((out[count:] == FILL).all()), "entries behind the list were written"


@pytest.mark.parametrize("n", [257, 262145])
def test_compaction_of_three_levels_equals_the_single_call_per_map(nm, cuda, n):
    import torch
    maps = [_dense_map(n, f) for f in ("some", "all", "none")]
    lib = nm.lib()
    nbytes = lib.nm_compact3_workspace_bytes(n)
    ws = _workspace(nbytes, cuda)
    tmaps = [_t(m, cuda) for m in maps]
    out = [torch.full((n + 1, 4), FILL, dtype=torch.float32, device=cuda) for _ in range(3)]
    cnt = torch.full((4,), -77, dtype=torch.int32, device=cuda)
    assert lib.nm_compact_keypoints3(_ptrs(tmaps), n, _ptrs(out), cnt.data_ptr(), ws.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == GUARD).all()) and int(cnt[3]) == -77
    for l in range(3):
        count, single = _compact_single(nm, cuda, maps[l])
        assert int(cnt[l]) == count == int((maps[l][:, 3] >= 0).sum())
        assert torch.equal(out[l], single), "level %d differs from the single call" % l


# (result width, result height, source width, source height)
@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (1, 1, 3, 3), (65, 5, 131, 11), (64, 4, 128, 8)])
def test_decimation_of_one_plane(nm, cuda, shape):
    import torch
    rw, rh, sw, sh = shape
    src = np.random.default_rng(rw * 131 + sh).random((sh, sw), dtype=np.float32)
    want = np.ascontiguousarray(src[0:2 * rh:2, 0:2 * rw:2])
    tsrc = _t(src, cuda)
    out = torch.full((rw * rh + 64,), FILL, dtype=torch.float32, device=cuda)
    assert nm.lib().nm_downsample2_f32(out.data_ptr(), rw, rh, tsrc.data_ptr(), sw, sh, None) == 0
    torch.cuda.synchronize()
    _same_bits(out[: rw * rh].reshape(rh, rw), want, "decimated plane")
    assert bool((out[rw * rh:] == FILL).all()), "wrote behind the result"
    _same_bits(nm.downsample2(tsrc, rw, rh), want, "downsample2")


def _planes(n, count, seed):
    rng = np.random.default_rng(seed)
    return [((rng.random(n, dtype=np.float32) - np.float32(0.5)) * np.float32(512.0)) for _ in range(count)]


@pytest.mark.parametrize("n", [1, 255, 257, 1048579])         # the last: one element past the 4096 workgroups of the single call
def test_subtract_of_one_plane(nm, cuda, n):
    import torch
    a, b = _planes(n, 2, n)
    ta, tb = _t(a, cuda), _t(b, cuda)
    out = torch.full((n + 64,), FILL, dtype=torch.float32, device=cuda)
    assert nm.lib().nm_subtract_f32(ta.data_ptr(), tb.data_ptr(), out.data_ptr(), n, 1, None) == 0
    torch.cuda.synchronize()
    _same_bits(out[:n], a - b, "A - B")
    assert bool((out[n:] == FILL).all()), "wrote behind the result"


def test_subtract_of_a_plane_batch_past_its_grid_cap(nm, cuda):
    import torch
    n = 524291                                                 # one element past 2048 workgroups per plane
    p = _planes(n, 4, 5)
    tp = [_t(x, cuda) for x in p]
    out = [torch.full((n + 64,), FILL, dtype=torch.float32, device=cuda) for _ in range(3)]
    assert nm.lib().nm_subtract_batch_f32(3, _ptrs(tp[1:]), _ptrs(tp[:3]), _ptrs(out), n, 1, None) == 0
    torch.cuda.synchronize()
    for k in range(3):
        _same_bits(out[k][:n], p[k + 1] - p[k], "plane %d" % k)
        assert bool((out[k][n:] == FILL).all()), "wrote behind result %d" % k
