"""The pair-batch convention on the MI355X (csrc/nm_pair_batch.hpp): the one count kernel through both of its callers, and the
slot tables at their seams -- the first slot of guided matching's second half launch (n = 33) and the last slot (n = 64) of
all four stages. Every pair's inputs depend on its index k, so a slot that lands on another pair changes the result.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = 64                                        # capA = capB of the seam tests
COUNT_CAP, COUNT_SIZES = 300, (0, 1, 300)        # one full 256-row tile + a ragged 44; more than one stride of the count loop


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _pair(k, rows):
    """Pair k: B holds A's rows in an order of its own, moved by a translation of its own (+ a little noise), so the right
    match of row i is perm[i] and every output depends on k. A few rows carry no match; the size is ragged in k."""
    rng = np.random.default_rng(7000 + k)
    perm = rng.permutation(rows)
    A = rng.integers(0, 4, (rows, 128)).astype(np.float32)
    ax, ay = (rng.uniform(0, 1000, rows).astype(np.float32) for _ in range(2))
    tx, ty = np.float32(k + 1), np.float32(2 * k + 1)
    B = np.empty_like(A)
    bx, by = np.empty_like(ax), np.empty_like(ay)
    B[perm] = A
    bx[perm] = ax + tx + rng.uniform(-0.25, 0.25, rows).astype(np.float32)
    by[perm] = ay + ty + rng.uniform(-0.25, 0.25, rows).astype(np.float32)
    m = perm.astype(np.int32)
    m[rng.permutation(rows)[:rows // 8]] = -1
    H = np.array([1, 0, tx + 0.5, 0, 1, ty - 0.5, 0, 0, 1], np.float32)
    return dict(A=A, ax=ax, ay=ay, B=B, bx=bx, by=by, m=m, H=H, nA=rows - k % 5, nB=rows)


def _lists(pairs, *keys):
    return [[p[key] for p in pairs] for key in keys]


def _upload(pairs, dev):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return [dict({key: t(p[key]) for key in ("A", "ax", "ay", "B", "bx", "by", "m")}, nA=t(np.array([p["nA"]], np.int32)),
                 nB=t(np.array([p["nB"]], np.int32))) for p in pairs]


def _np(out):
    """A wrapper's return tuple as numpy arrays (lists of per-pair tensors stacked)."""
    import torch
    torch.cuda.synchronize()
    return [np.stack([t.cpu().numpy() for t in o]) if isinstance(o, (list, tuple)) else o.cpu().numpy() for o in out]


def _assert_same(dev_out, host_out, what):
    assert len(dev_out) == len(host_out)
    for q, (d, h) in enumerate(zip(dev_out, host_out)):
        assert d.shape == h.shape and np.array_equal(_u32(d), _u32(h)), (what, "output %d" % q)


@pytest.fixture(scope="module")
def seam_pairs():
    return [_pair(k, ROWS) for k in range(64)]


@pytest.fixture(scope="module")
def seam_device(seam_pairs, cuda):
    return _upload(seam_pairs, cuda)


def test_the_count_kernel_through_both_callers(nm, cuda):
    import torch
    pairs = [dict(_pair(k, COUNT_CAP), nA=size, nB=COUNT_CAP) for k, size in enumerate(COUNT_SIZES)]
    up = _upload(pairs, cuda)
    H = np.stack([p["H"] for p in pairs])
    n, cap = len(pairs), COUNT_CAP
    g = nm.sift_match_guided_batch_dev(*_lists(up, "A", "ax", "ay", "nA", "B", "bx", "by", "nB"), torch.from_numpy(H).to(cuda),
                                       capA=cap, capB=cap, want_distance=True)
    u = nm.sift_match_mutual_batch_dev(*_lists(up, "A", "nA", "B", "nB", "m"), capA=cap, capB=cap, want_distance=True)
    for what, (results, count, _) in (("guided", g), ("mutual", u)):
        want = torch.stack([(results[k][:cap] >= 0).sum() for k in range(n)]).to(torch.int32)
        print(what, "counts", count.tolist())
        assert torch.equal(count, want), what
        assert count[0].item() == 0 and count[1].item() <= 1 and count[2].item() > cap // 2, what   # the sizes 0, 1 and 300
    _assert_same(_np(g), nm.sift_match_guided_host(*_lists(pairs, "A", "ax", "ay", "nA", "B", "bx", "by", "nB"), H, capA=cap,
                                                   capB=cap, want_distance=True), "guided")
    _assert_same(_np(u), nm.sift_match_mutual_host(*_lists(pairs, "A", "nA", "B", "nB", "m"), capA=cap, capB=cap,
                                                   want_distance=True), "mutual")


@pytest.mark.parametrize("n", [33, 64])
def test_guided_slots_at_the_seams(nm, cuda, seam_pairs, seam_device, n):
    import torch
    pairs, up = seam_pairs[:n], seam_device[:n]
    H = np.stack([p["H"] for p in pairs])
    dev = nm.sift_match_guided_batch_dev(*_lists(up, "A", "ax", "ay", "nA", "B", "bx", "by", "nB"), torch.from_numpy(H).to(cuda),
                                         capA=ROWS, capB=ROWS, want_distance=True)
    host = nm.sift_match_guided_host(*_lists(pairs, "A", "ax", "ay", "nA", "B", "bx", "by", "nB"), H, capA=ROWS, capB=ROWS,
                                     want_distance=True)
    assert len({host[0][k].tobytes() for k in range(n)}) == n              # no two pairs share a result
    _assert_same(_np(dev), host, "guided n = %d" % n)


def test_mutual_slots_at_the_last_seam(nm, cuda, seam_pairs, seam_device):
    dev = nm.sift_match_mutual_batch_dev(*_lists(seam_device, "A", "nA", "B", "nB", "m"), capA=ROWS, capB=ROWS, want_distance=True)
    host = nm.sift_match_mutual_host(*_lists(seam_pairs, "A", "nA", "B", "nB", "m"), capA=ROWS, capB=ROWS, want_distance=True)
    assert len({host[0][k].tobytes() for k in range(64)}) == 64
    _assert_same(_np(dev), host, "mutual n = 64")


def test_refit_slots_at_the_last_seam(nm, cuda, seam_pairs, seam_device):
    import torch
    H = np.stack([p["H"] for p in seam_pairs])
    dev = nm.ransac_refit_batch_dev(2, *_lists(seam_device, "ax", "ay", "nA", "bx", "by", "m"), torch.from_numpy(H).to(cuda),
                                    rounds=2, threshold=4.0, capA=ROWS, want_mask=True, want_rms=True)
    host = nm.ransac_refit_host(2, *_lists(seam_pairs, "ax", "ay", "nA", "bx", "by", "m"), H, rounds=2, threshold=4.0, capA=ROWS,
                                want_mask=True, want_rms=True)
    assert (host[2] == 1).all() and len({host[0][k].tobytes() for k in range(64)}) == 64
    _assert_same(_np(dev), host, "refit n = 64")


def test_ransac_slots_at_the_last_seam(nm, cuda, seam_device):
    seeds = [1000 + k for k in range(64)]
    args = lambda ps: _lists(ps, "ax", "ay", "nA", "bx", "by", "m")
    batch = _np(nm.ransac_batch_dev(2, *args(seam_device), iterations=16, threshold=4.0, seeds=seeds, capA=ROWS))
    assert (batch[3] == 1).all()
    for k in (0, 63):
        alone = _np(nm.ransac_batch_dev(2, *args(seam_device[k:k + 1]), iterations=16, threshold=4.0, seeds=seeds[k:k + 1], capA=ROWS))
        for q, (b, a) in enumerate(zip(batch, alone)):
            assert np.array_equal(_u32(b[k:k + 1]), _u32(a)), ("pair %d, output %d" % (k, q))
    assert len({batch[0][k].tobytes() for k in range(64)}) == 64           # 64 different maps
