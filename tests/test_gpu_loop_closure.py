"""The loop-closure path on rendered frames against the true maps (tests/loop_closure_ref.py): ten views of one texture on
a closed path, rendered on the device, through ingest -> detect -> select (keep 500) -> u8 finish, then

  a. the votes on those real rows against the numpy model and the host twin, entry for entry, under every split;
  b. the proposal against the true overlaps;
  c. the consecutive links, the proposed links and one wrong link through match -> mutual -> RANSAC -> refit -> refine ->
     verify in one batch;
  d. the refined maps against the float64 model of the refinement and against the truth;
  e. the adjustment over all links against its host twin, without the wrong link, against its float64 model and the truth;
  f. the blend of the plan's chain and of the adjusted chain against the scene;
  g. c .. f captured into one HIP graph and replayed on a second scene.

The chain runs once, in the module's fixture. The measured figures the bounds cite are in DESIGN.md section 7, "The loop-closure
path on rendered frames".
"""
import numpy as np
import pytest

import link_propose_ref as P
import link_refine_ref as RF
import loop_closure_ref as L
import mosaic_adjust_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
K, VW, VH = L.K, L.VW, L.VH
CAP, KEEP = 4096, 500                          # 500: a multiple of neither 32, 64 nor 256
SEEDS = (90, 91)
AMBIGUITY = 0.8
# The verification's overlap gate between the scene's two sides (0.10 and 0.35): its default, 0.60, is set for the linear pan
# of tests/test_gpu_link_verify.py, whose true links overlap by 0.82 .. 0.86.
MIN_OVERLAP = 0.5 * (L.LOW + L.HIGH)
# min_rows at the least the entry takes: the wrong link's few inlier rows would then count, so link_status alone keeps it out
ADJUST_ITERATIONS, MIN_ROWS = 16, 4
HIGH, LOW = L.high_pairs(), L.low_pairs()
CLOSURES = [p for p in HIGH if p[1] - p[0] >= 2]
WRONG = (0, 7)                                 # a strip of 0.09 of a frame in common: below any overlap worth linking
GEO = (VW, VH, L.SCENE_W, L.SCENE_H, L.ORIGIN_X, L.ORIGIN_Y)

# Measured on the MI355X over the 17 true links of scene 90; the bounds are four times these, for the
# u8-level quantisation of nml::pixel against the unquantised models on another scene seed.
REFINE_TO_MODEL_PX = 0.006554                  # largest corner distance, device's refined map to link_refine_ref.model_f64
ADJUST_TO_MODEL_PX = 8.6e-5                    # largest corner distance, device's adjusted maps to mosaic_adjust_ref.model_f64


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _feather():
    yy, xx = np.mgrid[0:VH, 0:VW]
    return (np.minimum(np.minimum(xx, VW - 1 - xx), np.minimum(yy, VH - 1 - yy)) / 64.0 + 0.01).astype(F32)


def _front(nm, dev, arenas, seed):
    """scene -> views rendered on the device -> gray -> detect -> the strongest KEEP rows -> u8 descriptors, as device tensors"""
    import torch
    scene = L.scene(seed)
    ds = _t(scene, dev)
    views = [nm.resample_perspective(ds, VW, VH, _t(np.linalg.inv(A).astype(F32), dev), inverse=True)[0] for A in L.view_maps()]
    grays = nm.ingest_batch(views)
    nm.detect_describe_batch(arenas, grays)
    sel = nm.sift_select_batch_dev([a.num_items for a in arenas], [a.x for a in arenas], [a.y for a in arenas], VW, VH,
                                   descs=[a.desc for a in arenas], keep=KEEP, capacity=CAP, want_index=False)
    count = sel["count"].clone()
    _, u8 = nm.desc_finish_batch_dev(sel["desc"], [count[k:k + 1] for k in range(K)], out_u8=True, capacity=CAP)
    torch.cuda.synchronize()
    return dict(scene=scene, views=views, grays=grays, x=sel["x"], y=sel["y"], u8=u8, count=count,
                detected=[int(a.num_items.item()) for a in arenas])


def _nearest_two_tie(descs, counts):
    """query rows, over all ordered frame pairs, whose two nearest candidates lie at one integer distance (float64 products of
    bytes are exact)"""
    rows = [d[:c].astype(np.float64) for d, c in zip(descs, counts)]
    sq = [(r * r).sum(1) for r in rows]
    ties = 0
    for a in range(len(rows)):
        for b in range(len(rows)):
            if a != b and counts[a] > 0 and counts[b] > 1:
                D = np.partition(sq[a][:, None] + sq[b][None, :] - 2.0 * (rows[a] @ rows[b].T), 1, axis=1)
                ties += int((D[:, 0] == D[:, 1]).sum())
    return ties


class _Back:
    """The post-proposal chain on a fixed link list, on the current stream, with its own input buffers and workspaces: match ->
    mutual -> RANSAC -> refit -> refine -> verify -> plan -> adjust -> place -> blend (the plan's chain and the adjusted one)."""
    NAMES = ("res", "mres", "mcount", "Hb", "rstatus", "H", "count", "st", "mask", "Hr", "str", "rstats", "ok", "why", "vstats",
             "records", "chain", "chain_out", "fstat", "rms", "astats", "placed", "extent", "canvas_plan", "wts_plan",
             "canvas_adj", "wts_adj")

    def __init__(self, nm, dev, la, lb, front):
        import torch
        self.nm, self.dev, self.la, self.lb = nm, dev, list(la), list(lb)
        n = len(la)
        self.inputs = {k: [t.clone() for t in front[k]] for k in ("views", "grays", "x", "y", "u8")}
        self.inputs["count"] = [front["count"].clone()]
        self.res = torch.empty((n, CAP), dtype=torch.int32, device=dev)
        self.mres = torch.empty((n, CAP), dtype=torch.int32, device=dev)
        self.mws = nm.MatchU8Workspace(n, CAP, CAP, dev)
        self.uws = nm.MatchMutualU8Workspace(n, CAP, CAP, dev)
        self.rws = nm.RansacBatchWorkspace(n, CAP, 2048, dev)
        self.lws = nm.LinkRefineWorkspace(n, dev)
        self.vws = nm.LinkVerifyWorkspace(n, dev)
        self.aws = nm.MosaicAdjustWorkspace(K, n, dev)
        self.plane = torch.full((VH, VW), 255, dtype=torch.uint8, device=dev)
        self.wts = _t(_feather(), dev)
        self.canvas = [torch.zeros((L.SCENE_H, L.SCENE_W, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.cwts = [torch.zeros((L.SCENE_H, L.SCENE_W), dtype=torch.float32, device=dev) for _ in range(2)]

    def load(self, front):
        for k, dst in self.inputs.items():
            for d, s in zip(dst, [front["count"]] if k == "count" else front[k]):
                d.copy_(s)

    def tables(self):
        i = self.inputs
        cnt = [i["count"][0][k:k + 1] for k in range(K)]
        la, lb = self.la, self.lb
        return dict(u8a=[i["u8"][a] for a in la], u8b=[i["u8"][b] for b in lb], na=[cnt[a] for a in la], nb=[cnt[b] for b in lb],
                    xa=[i["x"][a] for a in la], ya=[i["y"][a] for a in la], xb=[i["x"][b] for b in lb], yb=[i["y"][b] for b in lb],
                    ga=[i["grays"][a] for a in la], gb=[i["grays"][b] for b in lb])

    def adjust(self, pts, chain, mask, ok, links=None):
        """the adjustment over the first `links` links (default: all)"""
        n = len(self.la) if links is None else links
        return self.nm.mosaic_adjust(self.la[:n], self.lb[:n], *[p[:n] for p in pts], chain, VW, VH, mask=mask[:n], link_status=ok[:n],
                                     iterations=ADJUST_ITERATIONS, min_rows=MIN_ROWS, capA=CAP,
                                     workspace=self.aws if links is None else None)

    def enqueue(self):
        nm, t = self.nm, self.tables()
        n = len(self.la)
        self.res.fill_(-1)
        self.mres.fill_(-1)
        res, mres = list(self.res.unbind(0)), list(self.mres.unbind(0))
        nm.sift_match_u8_batch_dev(t["u8a"], t["na"], t["u8b"], t["nb"], results=res, ambiguity=AMBIGUITY, workspace=self.mws,
                                   capA=CAP, capB=CAP)
        _, mcount = nm.sift_match_mutual_u8_batch_dev(t["u8a"], t["na"], t["u8b"], t["nb"], res, capA=CAP, capB=CAP, results=mres,
                                                      workspace=self.uws)
        pts = (t["xa"], t["ya"], t["na"], t["xb"], t["yb"], mres)
        Hb, _, _, rstatus = nm.ransac_batch_dev(2, *pts, iterations=2048, threshold=1.0, seeds=list(range(n)), capA=CAP,
                                                workspace=self.rws)
        H, count, st, _, mask = nm.ransac_refit_batch_dev(2, *pts, Hb, status=rstatus, rounds=2, threshold=1.0, capA=CAP,
                                                          want_mask=True)
        Hr, str_, rstats = nm.link_refine_batch_dev(t["ga"], t["gb"], H, status=st, stride=4, iterations=4, workspace=self.lws)
        ok, why, vstats = nm.link_verify_batch_dev(t["ga"], t["gb"], Hr, status=str_, inliers=count, min_overlap=MIN_OVERLAP,
                                                   workspace=self.vws)
        records, chain, _ = nm.mosaic_plan(Hr[:K - 1], ok[:K - 1], *GEO)
        chain_out, fstat, rms, astats = self.adjust(pts, chain, mask, ok)
        placed, extent = nm.mosaic_place(chain_out, *GEO, frame_status=fstat)
        for c, w, rec in zip(self.canvas, self.cwts, (records, placed)):
            c.zero_()
            w.zero_()
            nm.transform_blend_batch(c, w, self.inputs["views"], self.plane, self.wts, rec)
        return (self.res, self.mres, mcount, Hb, rstatus, H, count, st, mask[:, :KEEP], Hr, str_, rstats, ok, why, vstats, records,
                chain, chain_out, fstat, rms, astats, placed, extent, self.canvas[0], self.cwts[0], self.canvas[1], self.cwts[1])

    def cover(self, records):
        """per frame, where it alone reaches the canvas under `records`"""
        import torch
        out = []
        for k in range(K):
            c, w = torch.zeros_like(self.canvas[0]), torch.zeros_like(self.cwts[0])
            self.nm.transform_blend_batch(c, w, [self.inputs["views"][k]], self.plane, self.wts, records[k:k + 1].contiguous())
            out.append((w != 0).cpu().numpy())
        return out


def _host(outs):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in zip(_Back.NAMES, outs)}


@pytest.fixture(scope="module")
def loop(nm, cuda):
    import torch
    arenas = [nm.SiftArena(VW, VH, CAP) for _ in range(K)]
    fronts = [_front(nm, cuda, arenas, seed) for seed in SEEDS]
    for a in arenas:
        a.close()
    f = fronts[0]
    counts = [int(v) for v in f["count"].cpu().numpy()]
    descs = [d.cpu().numpy() for d in f["u8"]]
    ties = _nearest_two_tie(descs, counts)
    if ties == 0:                             # the scene gave none: one row of frame 0 over another row of frame 0
        f["u8"][0][0].copy_(f["u8"][0][1])
        descs[0][0] = descs[0][1]
        ties = _nearest_two_tie(descs, counts)
    cnt = [f["count"][k:k + 1] for k in range(K)]
    votes = nm.link_votes_dev(f["u8"], cnt, ambiguity=AMBIGUITY, cap=CAP)
    torch.cuda.synchronize()
    votes_np = P.votes(descs, counts, CAP, AMBIGUITY)
    sc = P.scores(votes_np)
    hi, lo = min(sc[p] for p in HIGH), max(sc[p] for p in LOW)
    default = nm.link_rank_dev.__defaults__[0]
    min_votes = default if lo < default <= hi else max(1, (lo + hi + 1) // 2)
    ranked = nm.link_rank_dev(votes, min_votes=min_votes, min_gap=2)
    torch.cuda.synchronize()
    ranked = [r.cpu().numpy() for r in ranked]
    m = min(int(ranked[3][0]), 64 - K)
    proposed = [(int(a), int(b)) for a, b in zip(ranked[0][:m], ranked[1][:m])]      # read back: the client's choice, by design
    links = [(k, k + 1) for k in range(K - 1)] + proposed + [WRONG]
    back = _Back(nm, cuda, [a for a, _ in links], [b for _, b in links], f)
    out = _host(back.enqueue())
    cover = [back.cover(_t(out[k], cuda)) for k in ("records", "placed")]
    torch.cuda.synchronize()
    print("loop closure: detected %s, counts %s, %d ties, scores high >= %d, low <= %d, min_votes %d (default %d), proposed %s"
          % (f["detected"], counts, ties, hi, lo, min_votes, default, proposed))
    return dict(fronts=fronts, counts=counts, descs=descs, ties=ties, votes=votes.cpu().numpy(), votes_np=votes_np, hi=hi, lo=lo,
                min_votes=min_votes, default_min_votes=default, ranked=ranked, proposed=proposed, links=links, back=back, out=out,
                cover=cover, grays=[g.cpu().numpy() for g in f["grays"]], x=[t.cpu().numpy() for t in f["x"]],
                y=[t.cpu().numpy() for t in f["y"]])


def _true_links(loop):
    return range(len(loop["links"]) - 1)


def _tab(loop, n=None):
    """the refit-style tables of the first n links, read back: (src_x, src_y, nA, dst_x, dst_y, matches, mask) lists"""
    links = loop["links"][:n]
    o = loop["out"]
    return ([loop["x"][a] for a, _ in links], [loop["y"][a] for a, _ in links], [loop["counts"][a] for a, _ in links],
            [loop["x"][b] for _, b in links], [loop["y"][b] for _, b in links], [o["mres"][l] for l in range(len(links))],
            [np.pad(o["mask"][l], (0, CAP - KEEP)) for l in range(len(links))])


def _true_mosaic_maps():
    """G_k: view-k pixel -> mosaic (frame 0) coordinates"""
    A = L.view_maps()
    return np.stack([np.linalg.inv(A[0]) @ a for a in A])


# ---- a. votes ----

def test_votes_on_real_rows_equal_the_model_and_the_host_twin_under_every_split(nm, cuda, loop):
    import torch
    f = loop["fronts"][0]
    assert min(loop["counts"]) >= 300 and max(loop["counts"]) <= KEEP < CAP, loop["counts"]
    assert loop["ties"] > 0                  # the tie path is exercised: min1 == min2 on some query row
    host = nm.link_votes_host(loop["descs"], loop["counts"], ambiguity=AMBIGUITY, cap=CAP)
    assert np.array_equal(loop["votes_np"], host), np.argwhere(loop["votes_np"] != host)[:5]
    assert np.array_equal(loop["votes"], loop["votes_np"]), np.argwhere(loop["votes"] != loop["votes_np"])[:5]
    cnt = [f["count"][k:k + 1] for k in range(K)]
    try:
        for z in (0, 1, 3, K):
            nm.link_votes_set_split(z)
            got = nm.link_votes_dev(f["u8"], cnt, ambiguity=AMBIGUITY, cap=CAP)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            assert np.array_equal(got, loop["votes_np"]), (z, np.argwhere(got != loop["votes_np"])[:5])
    finally:
        nm.link_votes_set_split(0)


# ---- b. proposal ----

def test_proposal_is_the_high_overlap_pairs_beyond_the_sequence(nm, loop):
    sc = P.scores(loop["votes_np"])
    print("scores: high %s, low max %d" % (sorted(sc[p] for p in HIGH), loop["lo"]))
    assert loop["hi"] > loop["lo"], (loop["hi"], loop["lo"])
    assert loop["lo"] < loop["min_votes"] <= loop["hi"]
    la, lb, ls, cnt = loop["ranked"]
    want = sorted(CLOSURES, key=lambda p: (-sc[p], p))
    assert int(cnt[0]) == len(want) and loop["proposed"] == want, (loop["proposed"], want)
    assert [int(s) for s in ls[:len(want)]] == [sc[p] for p in want]
    for got, model, host in zip((la, lb, ls), P.rank(loop["votes_np"], loop["min_votes"], 2, 0, P.MAX_LINKS),
                                nm.link_rank_host(loop["votes"], min_votes=loop["min_votes"], min_gap=2)):
        assert np.array_equal(got, model) and np.array_equal(got, host)
    assert nm.link_rank_host(loop["votes"], min_votes=loop["min_votes"], min_gap=2)[3] == len(want)


# ---- c. the links through the chain ----

def test_true_links_verify_and_the_wrong_link_does_not(loop):
    o = loop["out"]
    assert loop["links"] == [(k, k + 1) for k in range(K - 1)] + loop["proposed"] + [WRONG]
    assert sorted(loop["proposed"]) == CLOSURES and max(L.overlap(*WRONG), L.overlap(*WRONG[::-1])) <= L.LOW
    true = list(_true_links(loop))
    print("inliers %s\noverlap %s\nncc %s\nwhy %s" % (o["count"].tolist(), np.round(o["vstats"][:, 2], 3).tolist(),
                                                       np.round(o["vstats"][:, 3], 4).tolist(), o["why"].tolist()))
    assert (o["rstatus"][true] == 1).all() and (o["st"][true] == 1).all() and (o["str"][true] == 1).all(), (o["st"], o["rstats"])
    assert (o["ok"][true] == 1).all() and (o["why"][true] == 0).all(), (o["why"], o["vstats"])
    assert o["ok"][-1] == 0 and o["why"][-1] != 0, (o["why"], o["vstats"][-1])
    for l, (a, b) in enumerate(loop["links"][:-1]):                 # the verification's overlap is the scene's, to a lattice step
        assert abs(o["vstats"][l, 2] - L.overlap(a, b)) < 0.02, (l, a, b, o["vstats"][l, 2], L.overlap(a, b))
    # direction: the refit's H of link (a, b) takes frame-a pixels to frame-b pixels. The reversed map is off by twice the
    # views' displacement, 270 px and more; the fit itself, extrapolated from the common part to the frame's corners, by a few.
    for l, (a, b) in enumerate(loop["links"][:-1]):
        assert RF.corner_error(o["H"][l], L.pair_map(a, b), VW, VH) < 20.0, (l, a, b)
        assert RF.corner_error(o["H"][l], L.pair_map(b, a), VW, VH) > 200.0, (l, a, b)


# ---- d. refinement ----

@pytest.fixture(scope="module")
def refine_models(loop):
    o = loop["out"]
    return [RF.model_f64(loop["grays"][a], loop["grays"][b], o["H"][l], stride=4, iterations=4)
            for l, (a, b) in enumerate(loop["links"][:-1])]


def test_refined_maps_against_the_float64_model_and_the_truth(loop, refine_models):
    o = loop["out"]
    bound = 4.0 * REFINE_TO_MODEL_PX
    rows = []
    for l, (a, b) in enumerate(loop["links"][:-1]):
        Ht = L.pair_map(a, b)
        rows.append((RF.corner_error(o["Hr"][l], refine_models[l], VW, VH), RF.corner_error(o["H"][l], Ht, VW, VH),
                     RF.corner_error(o["Hr"][l], Ht, VW, VH), RF.corner_error(refine_models[l], Ht, VW, VH)))
        print("link %2d (%d, %d): device to model %.5f px; to the truth: refit %.4f, refined %.4f, model %.4f px; %d steps, end %d"
              % ((l, a, b) + rows[-1] + (o["rstats"][l][6], o["rstats"][l][8])))
    d = np.array(rows)
    print("refinement: largest device-to-model distance %.6f px, bound %.6f px" % (d[:, 0].max(), bound))
    assert d[:, 0].max() <= bound, d[:, 0]
    assert (d[:, 2] <= d[:, 3] + bound).all(), d[:, 2:]


# ---- e. adjustment ----

@pytest.fixture(scope="module")
def adjust_model(loop):
    o = loop["out"]
    tab = _tab(loop)
    usable = [l for l in range(len(loop["links"])) if o["ok"][l] == 1]
    links = [loop["links"][l] + R.inlier_points(tab, l) for l in usable]
    assert all(len(p) >= MIN_ROWS for _, _, p, _ in links)
    return R.model_f64(R.chain_to_maps(o["chain"]), links, VW, VH, anchor=0)


def test_adjustment_equals_its_host_twin(nm, loop):
    o = loop["out"]
    tab = _tab(loop)
    la, lb = [a for a, _ in loop["links"]], [b for _, b in loop["links"]]
    want = nm.mosaic_adjust_host(la, lb, *tab[:6], o["chain"], VW, VH, mask=np.stack(tab[6]), link_status=o["ok"],
                                 iterations=ADJUST_ITERATIONS, min_rows=MIN_ROWS, capA=CAP)
    for name, w in zip(("chain_out", "fstat", "rms", "astats"), want):
        assert np.array_equal(bits(o[name]), bits(w)), (name, o[name], w)
    print("adjustment stats %s" % dict(zip(nm.MOSAIC_ADJUST_STATS, o["astats"].tolist())))
    assert int(o["astats"][7]) == R.END_CONVERGED and o["astats"][5] >= 1, o["astats"]
    assert int(o["astats"][3]) == len(loop["links"]) - 1 and (o["fstat"] == 1).all(), (o["astats"], o["fstat"])
    # ragged tables: every count is below the capacity, and the refit's mask drops rows the matcher kept
    matched = np.array([(tab[5][l][:tab[2][l]] >= 0).sum() for l in range(len(la))])
    kept = np.array([tab[6][l].sum() for l in range(len(la))])
    assert (kept[:-1] < matched[:-1]).any() and (kept <= matched).all(), (kept, matched)


def test_adjustment_ignores_the_wrong_link(nm, cuda, loop):
    import torch
    o, back = loop["out"], loop["back"]
    n = len(loop["links"])
    assert o["ok"][-1] == 0 and o["mask"][-1].sum() >= MIN_ROWS      # a link that would count were its status not read
    assert not o["rms"][-1].any() and o["rms"][:-1].all(), o["rms"]
    back.load(loop["fronts"][0])
    t = back.tables()
    pts = (t["xa"], t["ya"], t["na"], t["xb"], t["yb"], [_t(o["mres"][l], cuda) for l in range(n)])
    mask = _t(np.pad(o["mask"], ((0, 0), (0, CAP - KEEP))), cuda)
    got = back.adjust(pts, _t(o["chain"], cuda), mask, _t(o["ok"], cuda), links=n - 1)
    torch.cuda.synchronize()
    for name, g in zip(("chain_out", "fstat", "rms", "astats"), got):
        want = o[name][:n - 1] if name == "rms" else o[name]
        assert np.array_equal(bits(g.cpu().numpy()), bits(want)), name


def test_adjusted_maps_against_the_float64_model(loop, adjust_model):
    o = loop["out"]
    G = R.chain_to_maps(o["chain_out"])
    d = R.corner_error(G, adjust_model, VW, VH)
    bound = 4.0 * ADJUST_TO_MODEL_PX
    print("adjustment: device to model %.6f px, bound %.6f px" % (d, bound))
    assert d <= bound, d


def _truth_figures(Gs):
    Gt = _true_mosaic_maps()
    return (R.loop_gap(Gs, L.pair_map(K - 1, 0), VW, VH), float(np.mean([R.corner_error([g], [t], VW, VH) for g, t in zip(Gs, Gt)])),
            R.corner_error(Gs, Gt, VW, VH))


def _chain_of(H):
    """the maps G_k of the sequential links H (frame k -> frame k + 1) multiplied up, as the plan does"""
    M, out = np.eye(3), [np.eye(3)]
    for h in np.asarray(H, np.float64).reshape(-1, 3, 3):
        M = h @ M
        out.append(np.linalg.inv(M / M[2, 2]))
    return np.stack([g / g[2, 2] for g in out])


def test_adjustment_closes_the_loop_and_follows_its_model_away_from_the_truth(loop, adjust_model):
    """The loop gap over the true closing map falls, as it should. The mean corner error against the true maps does NOT:
    measured on the MI355X, scene 90 (loop gap / mean / largest corner error, px):

        the refit's links multiplied up (reported)       9.3692 / 4.9359 / 10.1080
        plan's chain (the refined links multiplied up)   0.3679 / 0.3311 / 0.8515
        adjusted, device                                 0.1064 / 1.7496 / 5.1569
        adjusted, float64 model of the same cost         0.1064 / 1.7496 / 5.1570

    The independent float64 model lands where the device does (8.6e-5 px apart), so this is what the cost's minimum is on
    this scene, not an error of the kernels: the cost sees keypoint coordinates alone, about 90 inlier rows per link inside
    the 0.42 of a frame two views share. It betters the chain of the keypoint fits it is made of, and gives up the
    photometric refinement's few hundredths of a pixel per link. What is asserted is what holds: the
    gap falls, and the device's three figures are the exact minimiser's to the device-to-model bound."""
    o = loop["out"]
    chains = (("plan's chain", R.chain_to_maps(o["chain"])), ("adjusted", R.chain_to_maps(o["chain_out"])),
              ("float64 model", adjust_model), ("refit's chain", _chain_of(o["H"][:K - 1])))
    fig = {what: _truth_figures(G) for what, G in chains}
    for what, v in fig.items():
        print("%-14s loop gap %.4f px, mean corner error %.4f px, largest %.4f px" % ((what,) + v))
    before, after, model = fig["plan's chain"], fig["adjusted"], fig["float64 model"]
    bound = 4.0 * ADJUST_TO_MODEL_PX
    assert after[0] < before[0], (before, after)
    assert all(abs(a - m) <= bound for a, m in zip(after, model)), (after, model)


# ---- f. blend ----

def test_blend_of_both_chains_against_the_scene(loop):
    o = loop["out"]
    scene = loop["fronts"][0]["scene"][..., :3].astype(int)
    both, med = [], []
    for canvas, cover in zip((o["canvas_plan"], o["canvas_adj"]), loop["cover"]):
        multi = np.sum(cover, axis=0) >= 2
        assert multi.sum() > 0.2 * L.SCENE_W * L.SCENE_H
        diff = np.abs(canvas[..., :3].astype(int) - scene)
        med.append(float(np.median(diff[multi])))
        both.append(cover[0] & cover[K - 1])
    region = both[0] & both[1]
    assert region.sum() > 0.3 * VW * VH, region.sum()
    ends = [float(np.median(np.abs(c[..., :3].astype(int) - scene)[region])) for c in (o["canvas_plan"], o["canvas_adj"])]
    means = [float(np.mean(np.abs(c[..., :3].astype(int) - scene)[region])) for c in (o["canvas_plan"], o["canvas_adj"])]
    print("blend: median |canvas - scene| where two frames met: plan %.1f, adjusted %.1f; where views 0 and %d met: plan %.1f "
          "(mean %.3f), adjusted %.1f (mean %.3f)" % (med[0], med[1], K - 1, ends[0], means[0], ends[1], means[1]))
    assert max(med) <= 3, med
    assert ends[1] <= ends[0], ends
    assert (o["records"][:, 13] == 1).all() and (o["placed"][:, 13] == 1).all()


# ---- g. capture ----

def test_post_proposal_chain_in_one_graph_replays_on_the_second_scene(nm, cuda, loop):
    import torch
    back = loop["back"]
    back.load(loop["fronts"][0])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        warm = back.enqueue()                              # warm-up outside capture
    warm = _host(warm)
    for k, v in loop["out"].items():                       # and the fixture's run repeats bit for bit
        assert np.array_equal(bits(warm[k]), bits(v)), k
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = back.enqueue()
    back.load(loop["fronts"][1])
    torch.cuda.synchronize()
    g.replay()
    got = _host(captured)
    with torch.cuda.stream(s):
        want = back.enqueue()
    want = _host(want)
    for k in _Back.NAMES:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    n = len(loop["links"])
    assert (got["ok"][:n - 1] == 1).all() and got["ok"][-1] == 0, (got["why"], got["vstats"])
    assert int(got["astats"][7]) == R.END_CONVERGED and got["canvas_adj"].any()
    assert not np.array_equal(got["Hr"], loop["out"]["Hr"])
