"""Direct link refinement on the device (nm_link_refine_batch_dev_f32): equal to the host twin bit for bit on every output,
independent of a pair's slot, of n and of what the outputs and the workspace held, equal at shapes where the tile walk
wraps, and capturable between the refit and the verification."""
import numpy as np
import pytest

from test_gpu_link_verify import SCENE_H, SCENE_W, VH, VW, _Chain, _t, _views
from test_link_refine_host import FRAMES, MAPS, MODELS, START, disc, frame, moved, smooth
import link_refine_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32


def _same(dev_out, host_out):
    H, st, stats = (o.cpu().numpy() for o in dev_out)
    return (np.array_equal(H.view(np.uint32), host_out[0].view(np.uint32)) and np.array_equal(st, host_out[1]) and
            np.array_equal(stats.view(np.uint64), host_out[2].view(np.uint64)))


def _both(nm, dev, As, Bs, H, **kw):
    """(device outputs, host twin outputs) of one call; frames are uploaded once each (repeated arrays share a tensor)"""
    up = {}
    for a in list(As) + list(Bs):
        if id(a) not in up:
            up[id(a)] = _t(a, dev)
    dkw = {k: (_t(np.asarray(v, F32 if k == "mask" else np.int32), dev) if k in ("mask", "status") and v is not None else v)
           for k, v in kw.items()}
    got = nm.link_refine_batch_dev([up[id(a)] for a in As], [up[id(b)] for b in Bs], _t(np.asarray(H, F32), dev), **dkw)
    return got, nm.link_refine_host(As, Bs, H, **kw)


def _pairs(size, n):
    """n pairs over five frames of one size: B is A moved and brightened (even pairs) or another frame (odd pairs), the
    starts in turn: near the truth, the identity, a homography, a map wholly outside B, a NaN."""
    fw, fh = size
    frames = [(0.5 * frame(10 + k, fw, fh) + 0.5 * smooth(fw, fh, 3.0 * k, k)).astype(F32) for k in range(5)]
    shifted = [moved(f) for f in frames]
    nan = np.eye(3, dtype=F32).reshape(9)
    nan[7] = np.nan
    maps = [START.reshape(9), np.eye(3, dtype=F32).reshape(9), np.asarray(MAPS["homography"], F32).reshape(9),
            np.asarray(MAPS["outside"], F32).reshape(9), START.reshape(9), nan, START.reshape(9)]
    return ([frames[k % 5] for k in range(n)], [shifted[k % 5] if k % 2 == 0 else frames[(k + 1) % 5] for k in range(n)],
            np.stack([maps[k % len(maps)] for k in range(n)]), [int(k % 11 != 9) for k in range(n)])


@pytest.mark.parametrize("size", FRAMES)
@pytest.mark.parametrize("n", [1, 2, 33, 64])
def test_device_equals_host_twin(nm, cuda, size, n):
    As, Bs, H, status = _pairs(size, n)
    ends = set()
    for model, iterations, stride, mask in ((R.TRANSLATION, 1, 1, None), (R.AFFINE, 4, 2, disc(*size)),
                                            (R.HOMOGRAPHY, 4, 1, None), (R.HOMOGRAPHY, 1, 3, disc(*size)),
                                            (R.TRANSLATION, 4, 7, None), (R.AFFINE, 8, 1, None), (R.HOMOGRAPHY, 4, 64, None)):
        got, want = _both(nm, cuda, As, Bs, H, status=status, mask=mask, model=model, stride=stride, iterations=iterations,
                          min_pixels=20, max_step=4.0)
        assert _same(got, want), (size, n, model, iterations, stride, want[2])
        ends |= set(want[2][:, 8].astype(int).tolist())
    if n >= 33:                                            # pairs of these calls ended for different reasons
        assert {R.END_ITERATIONS, R.END_CONVERGED, R.END_UNUSABLE, R.END_FEW_PIXELS} <= ends, ends


def test_pairs_of_one_call_end_for_different_reasons(nm, cuda):
    fw, fh = 64, 48
    A = smooth(fw, fh)
    B = moved(A)
    flat = np.full_like(A, 100)
    far = (0.5 * A + 0.5 * np.roll(A, 9, 1)).astype(F32)          # no map near START explains it: the first step is large
    I = np.eye(3, dtype=F32).reshape(9)
    S = START.reshape(9)
    As = [A, A, flat, A, A, A]
    Bs = [B, B, flat, A, B, far]
    H = np.stack([S, S, I, I, S, S])
    kw = dict(status=[0, 1, 1, 1, 1, 1], stride=1, iterations=2, min_pixels=64, max_step=0.3)
    got, want = _both(nm, cuda, As, Bs, H, **kw)
    assert _same(got, want), want[2]
    ends = want[2][:, 8].astype(int).tolist()
    assert ends[:4] == [R.END_UNUSABLE, R.END_STEP, R.END_SINGULAR, R.END_CONVERGED], want[2]
    got, want = _both(nm, cuda, As, Bs, H, **dict(kw, max_step=8.0))
    assert _same(got, want), want[2]
    ends = want[2][:, 8].astype(int).tolist()
    assert ends[1] == R.END_ITERATIONS and want[1].tolist() == [0, 1, 0, 1, 1, 1] and want[2][1, 6] == 2, want[2]
    got, want = _both(nm, cuda, As, Bs, H, **dict(kw, min_pixels=62 * 46 + 1))
    assert _same(got, want) and set(want[2][1:, 8]) == {R.END_FEW_PIXELS}


def _raw(nm, dev, As, Bs, H, ws, fill, **kw):
    """The C entry on outputs and a workspace filled with the byte `fill` beforehand: (H_out, status, stats) as numpy."""
    import torch
    n = len(As)
    fh, fw = As[0].shape
    H_out = torch.empty((n, 9), dtype=torch.float32, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    stats = torch.empty((n, 9), dtype=torch.float64, device=dev)
    for t in (H_out, st, stats, ws.buf):
        t.view(torch.uint8).fill_(fill)
    rc = nm.lib().nm_link_refine_batch_dev_f32(n, nm._pair_dev_table(As, torch.float32), nm._pair_dev_table(Bs, torch.float32),
                                               fw, fh, None, H.data_ptr(), None, kw["model"], kw["stride"], kw["iterations"],
                                               kw["min_pixels"], kw["max_step"], H_out.data_ptr(), st.data_ptr(),
                                               stats.data_ptr(), ws.buf.data_ptr(), nm._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in (H_out, st, stats)]


def test_outputs_do_not_depend_on_slot_n_or_earlier_contents(nm, cuda):
    fw, fh = 131, 97
    A = (0.5 * frame(30, fw, fh) + 0.5 * smooth(fw, fh)).astype(F32)
    P = (A, moved(A), START.reshape(9))
    kw = dict(model=R.HOMOGRAPHY, stride=2, iterations=4, min_pixels=64, max_step=8.0)
    want = nm.link_refine_host([P[0]], [P[1]], P[2][None], **kw)
    assert want[1][0] == 1 and want[2][0][6] >= 2
    dA, dB, dH = _t(P[0], cuda), _t(P[1], cuda), _t(P[2][None], cuda)
    ws1, ws64 = nm.LinkRefineWorkspace(1, cuda), nm.LinkRefineWorkspace(64, cuda)
    alone = _raw(nm, cuda, [dA], [dB], dH, ws1, 0xFF, **kw)
    assert _same([_t(o, "cpu") for o in alone], want)
    again = _raw(nm, cuda, [dA], [dB], dH, ws1, 0x5A, **kw)     # a second run over other sentinels
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(alone, again))
    rep = _raw(nm, cuda, [dA] * 64, [dB] * 64, dH.repeat(64, 1), ws64, 0xFF, **kw)      # repeated pointers
    assert all(np.array_equal(r.view(np.uint8).reshape(64, -1), np.tile(a.view(np.uint8).reshape(1, -1), (64, 1)))
               for r, a in zip(rep, alone))
    As, Bs, H, _ = _pairs((fw, fh), 64)
    dAs, dBs = [_t(a, cuda) for a in As[:5]], {id(b): _t(b, cuda) for b in Bs[:10]}
    for slot in (0, 31, 32, 63):
        a, b, h = [dAs[k % 5] for k in range(64)], [dBs[id(Bs[k])] for k in range(64)], H.copy()
        a[slot], b[slot], h[slot] = dA, dB, P[2]
        got = _raw(nm, cuda, a, b, _t(h, cuda), ws64, 0xFF, **kw)
        assert all(np.array_equal(g[slot:slot + 1].view(np.uint8), o.view(np.uint8)) for g, o in zip(got, alone)), slot


@pytest.mark.parametrize("size,iterations", [((1920, 1080), 2), ((1000, 600), 3)])
def test_shapes_where_the_tile_walk_wraps_equal_host_twin(nm, cuda, size, iterations):
    """More than 256 lattice tiles at stride 1 (1920 x 1080: 30 x 34; 1000 x 600: 16 x 19, the last tile column 40 lattice
    columns wide), so virtual workgroups own several tiles."""
    fw, fh = size
    assert -(-fw // 64) * -(-fh // 32) > 256
    rng = np.random.default_rng(fw)
    yy, xx = np.mgrid[0:fh, 0:fw]
    A = (120 + 50 * np.sin(xx / 9.0) * np.cos(yy / 11.0) + 30 * np.sin((xx + 2 * yy) / 23.0) +
         20 * rng.random((fh, fw))).astype(F32)
    B = np.clip(0.9 * (0.5 * np.roll(A, (3, -5), (0, 1)) + 0.5 * np.roll(A, (4, -4), (0, 1))) + 7, 0, 255).astype(F32)
    A[5, 7], B[100, 200], B[fh - 1, fw - 1] = np.nan, 300.0, -1.0
    H = np.array([[1.0001, 0.0002, -4.2], [-0.0001, 0.9999, 3.1], [1e-7, -2e-7, 1]], F32).reshape(1, 9)
    got, want = _both(nm, cuda, [A], [B], H, stride=1, iterations=iterations, max_step=8.0)
    assert _same(got, want), want
    assert want[1][0] == 1 and want[2][0, 0] > 0.9 * fw * fh and want[2][0, 6] == iterations


# ---- the chain: .. -> refit -> refine -> verify -> plan ----

class _RefinedChain(_Chain):
    def __init__(self, nm, dev):
        super().__init__(nm, dev)
        self.lws = nm.LinkRefineWorkspace(7, dev)

    def enqueue(self, views):
        nm = self.nm
        A, B = self.arenas[:-1], self.arenas[1:]
        grays = nm.ingest_batch(views)
        nm.detect_describe_batch(self.arenas, grays)
        pts = ([a.x for a in A], [a.y for a in A], [a.num_items for a in A], [b.x for b in B], [b.y for b in B], self.res)
        nm.sift_match_batch_dev([a.desc for a in A], [a.num_items for a in A], [b.desc for b in B],
                                [b.num_items for b in B], self.res, 0.8, workspace=self.mws)
        Hb, _, _, status = nm.ransac_batch_dev(2, *pts, iterations=2048, threshold=1.0, seeds=list(range(7)), capA=CAP_,
                                               workspace=self.rws)
        H, count, st, _ = nm.ransac_refit_batch_dev(2, *pts, Hb, status=status, rounds=2, threshold=1.0, capA=CAP_)
        Hr, str_, rstats = nm.link_refine_batch_dev(grays[:-1], grays[1:], H, status=st, stride=4, iterations=4,
                                                    workspace=self.lws)
        ok, why, stats = nm.link_verify_batch_dev(grays[:-1], grays[1:], Hr, status=str_, inliers=count, workspace=self.vws)
        records, chain, _ = nm.mosaic_plan(Hr, ok, VW, VH, SCENE_W, SCENE_H, 40, 64)
        return H, count, st, Hr, str_, rstats, ok, why, stats, records, chain


CAP_ = 8192


def test_chain_with_refinement_captures_and_replays(nm, oracle, cuda):
    import torch
    v1, v2 = _views(nm, cuda, 90), _views(nm, cuda, 91)
    bufs = [v.clone() for v in v1]
    ch = _RefinedChain(nm, cuda)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ch.enqueue(bufs)                                  # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = ch.enqueue(bufs)
    for b, v in zip(bufs, v2):
        b.copy_(v)
    for r in ch.res:
        r.fill_(-1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = [o.cpu().numpy().copy() for o in captured]
    for r in ch.res:
        r.fill_(-1)
    with torch.cuda.stream(s):
        want = ch.enqueue([v.clone() for v in v2])
    torch.cuda.synchronize()
    want = [o.cpu().numpy().copy() for o in want]
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    H, count, st, Hr, str_, rstats, ok, why, stats, records, chain = got
    assert (st == 1).all() and (str_ == 1).all() and (ok == 1).all() and (why == 0).all(), (rstats, why)
    assert (records.view(np.int32).reshape(8, 16)[:, 13] == 1).all()
    # today's chain, run beside it on the same views: the refit's outputs are the same, the refinement is an added stage
    for r in ch.res:
        r.fill_(-1)
    with torch.cuda.stream(s):
        plain = _Chain.enqueue(ch, [v.clone() for v in v2])
    torch.cuda.synchronize()
    assert np.array_equal(plain[0].cpu().numpy().view(np.uint32), H.view(np.uint32))
    assert np.array_equal(plain[1].cpu().numpy(), count) and (plain[2].cpu().numpy() == 1).all()
    # the refit's and the refined maps against the views' true maps: the refined map is no farther from the truth than the
    # unquantised float64 model's, run on the same gray planes from the refit's map, plus the device-to-model bound of
    # tests/test_gpu_loop_closure.py
    from test_gpu_loop_closure import REFINE_TO_MODEL_PX
    from test_link_refine_host import true_maps
    grays = [g.cpu().numpy() for g in nm.ingest_batch([v.clone() for v in v2])]
    for k, Ht in enumerate(true_maps()):
        model = R.model_f64(grays[k], grays[k + 1], H[k], stride=4, iterations=4)
        e0, e1, em = (R.corner_error(m, Ht, VW, VH) for m in (H[k], Hr[k], model))
        print("link %d: refit %.4f px, refined %.4f px, model %.4f px, device to model %.5f px, %d steps, end %d"
              % (k, e0, e1, em, R.corner_error(Hr[k], model, VW, VH), rstats[k][6], rstats[k][8]))
        assert e1 <= em + 4.0 * REFINE_TO_MODEL_PX, (k, e1, em)
    ch.close()
