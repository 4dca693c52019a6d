"""The descriptor finish on the GPU (nm_sift_desc_finish_batch_dev) against its host twin, bit for bit: 1, 3 and 64 frames
in one launch, counts around the wave and workgroup sizes, at and above the capacity, both modes, every output set
(f32, u8, both, f32 in place), sentinel-filled outputs that rows at and beyond the count must leave alone, and the
refusals with live device pointers.
"""
import ctypes as C

import numpy as np
import pytest

from test_desc_finish_host import edge_rows, golden_rows, random_rows

pytestmark = pytest.mark.gpu

CAP = 130
COUNTS = (0, 1, 63, 64, 65, CAP, CAP + 70, 3, 129, -2)

_pool = None


def pool():
    global _pool
    if _pool is None:
        _pool = np.concatenate([edge_rows(), golden_rows(), random_rows(5, 200)])
    return _pool


def frames(n):
    p = pool()
    descs = [np.ascontiguousarray(np.roll(p, -17 * k, 0)[:CAP]) for k in range(n)]
    counts = [COUNTS[k % len(COUNTS)] for k in range(n)]
    if n == 1:
        counts = [CAP]
    return descs, counts


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 64])
def test_device_equals_host_twin(nm, cuda, n, mode):
    import torch
    descs, counts = frames(n)
    host_f, host_u = nm.desc_finish_host(descs, counts, mode=mode, capacity=CAP)
    d_descs = [torch.from_numpy(d).to(cuda) for d in descs]
    d_counts = [torch.tensor([c], dtype=torch.int32, device=cuda) for c in counts]
    kept = [min(max(c, 0), CAP) for c in counts]
    for outputs in ("f32", "u8", "both", "aliased"):
        src = [d.clone() for d in d_descs]
        f = [torch.full((CAP, 128), -7.0, dtype=torch.float32, device=cuda) for _ in range(n)] if outputs in ("f32", "both") else None
        u = [torch.full((CAP, 128), 7, dtype=torch.uint8, device=cuda) for _ in range(n)] if outputs in ("u8", "both", "aliased") else None
        if outputs == "aliased":
            f = src
        got_f, got_u = nm.desc_finish_batch_dev(src, d_counts, mode=mode, out_f32=f, out_u8=u, capacity=CAP)
        torch.cuda.synchronize()
        for k in range(n):
            if got_f is not None:
                g = got_f[k].cpu().numpy()
                assert np.array_equal(g[:kept[k]].view(np.uint32), host_f[k, :kept[k]].view(np.uint32)), (outputs, k, counts[k])
                rest = descs[k][kept[k]:] if outputs == "aliased" else np.full((CAP - kept[k], 128), -7.0, np.float32)
                assert np.array_equal(g[kept[k]:].view(np.uint32), rest.view(np.uint32)), (outputs, k, "rows beyond the count")
            if got_u is not None:
                g = got_u[k].cpu().numpy()
                assert np.array_equal(g[:kept[k]], host_u[k, :kept[k]]), (outputs, k, counts[k])
                assert (g[kept[k]:] == 7).all(), (outputs, k, "rows beyond the count")
            if outputs != "aliased":
                assert np.array_equal(src[k].cpu().numpy().view(np.uint32), descs[k].view(np.uint32))   # the input is read only


def test_new_outputs_and_a_smaller_capacity(nm, cuda):
    import torch
    descs, _ = frames(3)
    d = [torch.from_numpy(x).to(cuda) for x in descs]
    cnt = [torch.tensor([c], dtype=torch.int32, device=cuda) for c in (100, 40, 90)]
    f, u = nm.desc_finish_batch_dev(d, cnt, mode="root", out_f32=True, out_u8=True, capacity=64)
    hf, hu = nm.desc_finish_host(descs, [100, 40, 90], mode="root", capacity=64)
    torch.cuda.synchronize()
    assert f[0].shape == (64, 128) and u[0].dtype == torch.uint8
    for k in range(3):
        assert np.array_equal(f[k].cpu().numpy().view(np.uint32), hf[k].view(np.uint32)) and np.array_equal(u[k].cpu().numpy(), hu[k])
    only_u = nm.desc_finish_batch_dev(d, cnt, out_u8=True)
    assert only_u[0] is None and only_u[1][0].shape == (CAP, 128)


def test_refusals_touch_nothing(nm, cuda):
    import torch
    lib = nm.lib()
    d = torch.ones((8, 128), dtype=torch.float32, device=cuda)
    cnt = torch.tensor([8], dtype=torch.int32, device=cuda)
    f = torch.full((8, 128), -7.0, dtype=torch.float32, device=cuda)
    u = torch.full((8, 128), 7, dtype=torch.uint8, device=cuda)
    tab = lambda t, k=2: (C.c_void_p * 64)(*([t.data_ptr()] * k))
    st = torch.cuda.current_stream().cuda_stream

    def call(n=2, cap=8, mode=0, **kw):
        a = dict(desc=tab(d), num=tab(cnt), f=tab(f), u=tab(u))
        a.update(kw)
        return lib.nm_sift_desc_finish_batch_dev(n, a["desc"], a["num"], cap, a["f"], a["u"], mode, st)

    for kw in (dict(n=0), dict(n=65), dict(cap=0), dict(cap=1 << 22), dict(mode=2), dict(desc=None), dict(num=None),
               dict(f=None, u=None), dict(desc=tab(d, 1)), dict(num=tab(cnt, 1)), dict(f=tab(f, 1)), dict(u=tab(u, 1))):
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    assert (f == -7.0).all() and (u == 7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (u == 45).all()
    for kw in (dict(out_f32=None, out_u8=None), dict(out_u8=True, mode=5), dict(out_u8=True, capacity=9),
               dict(out_u8=[u, u]), dict(out_u8=[u.cpu()])):
        with pytest.raises(nm.NmError):
            nm.desc_finish_batch_dev([d], [cnt], **kw)
