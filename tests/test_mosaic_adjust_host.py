"""The global mosaic adjustment on the host (nm_mosaic_adjust_host_f32, nm_mosaic_adjust_sums_host_f32) and the placement on
a given chain (nm_mosaic_place_host_f32): the sums against their numpy restatement bit for bit, a loop of 12 frames against
an independent float64 model, every end reason, the participation rules and every refusal."""
import numpy as np
import pytest

import mosaic_adjust_ref as R

F32, F64 = np.float32, np.float64
FW, FH = R.FW, R.FH

# The loop of R.scene() (seed 5, noise 0.3 px), measured with model_f64: largest corner error against the truth 1.832 px
# before and 1.401 px after, loop gap 0.413 px before and 0.301 px after. The bars are twice the model's after-values, as
# NCC_ALLOWANCE was set. The host twin lay 4.9e-5 px from the model (largest corner distance of any frame).
MODEL_CORNER_AFTER, MODEL_GAP_AFTER, TWIN_TO_MODEL = 1.401, 0.301, 4.9e-5
CORNER_BAR, GAP_BAR = 2 * MODEL_CORNER_AFTER, 2 * MODEL_GAP_AFTER


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def loop(nm):
    G, la, lb, tab = R.scene()
    n, L = len(G), len(la)
    Ht = np.stack([np.linalg.inv(G[b]) @ G[a] for a, b in zip(la, lb)])
    Ht = (Ht / Ht[:, 2:, 2:]).astype(F32).reshape(L, 9)
    H, count, st, _, mask = nm.ransac_refit_host(2, *tab[:6], Ht, rounds=2, threshold=4.0, want_mask=True)
    assert st.all() and (count >= 290).all()
    records, chain, extent = nm.mosaic_plan_host(H[:n - 1], None, FW, FH, 2000, 1500, 700, 500)
    return dict(G=G, la=la, lb=lb, tab=tab[:6], mask=mask, H=H, chain=chain, n=n, L=L)


def adjust(nm, s, **kw):
    kw.setdefault("mask", s["mask"])
    return nm.mosaic_adjust_host(kw.pop("la", s["la"]), kw.pop("lb", s["lb"]), *kw.pop("tab", s["tab"]),
                                 kw.pop("chain", s["chain"]), FW, FH, **kw)


def pair_case(seed, m=12):
    """two frames, one link of m exact points under a far map, both frames starting at the identity"""
    rng = np.random.default_rng(seed)
    p = rng.random((m, 2)) * [FW, FH]
    th = rng.uniform(0.5, 3.0)
    Ht = np.array([[np.cos(th), -np.sin(th), rng.uniform(-200, 200)], [np.sin(th), np.cos(th), rng.uniform(-200, 200)],
                   [rng.uniform(-1e-3, 1e-3), rng.uniform(-1e-3, 1e-3), 1]])
    q = R.apply(Ht, p)
    tab = [[p[:, 0].astype(F32)], [p[:, 1].astype(F32)], [m], [q[:, 0].astype(F32)], [q[:, 1].astype(F32)],
           [np.arange(m, dtype=np.int32)]]
    return tab, np.tile(np.eye(3, dtype=F32).reshape(1, 9), (2, 1))


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 511, 512, 513, 1100])
def test_sums_equal_numpy_restatement(nm, rows):
    rng = np.random.default_rng(rows)
    cap = max(rows, 1) + 3
    sx, sy = (rng.random(cap) * FW).astype(F32), (rng.random(cap) * FH).astype(F32)
    dx, dy = (rng.random(cap) * FW).astype(F32), (rng.random(cap) * FH).astype(F32)
    mt = rng.permutation(cap).astype(np.int32)
    G = R.true_maps()
    Ga, Gb = R.normalised(G[2], FW, FH), R.normalised(G[5], FW, FH)
    mask = (rng.random(cap) < 0.7).astype(np.uint8)
    holes = mt.copy()
    holes[::5] = -1
    neg = sx.copy()
    neg[1::7] = -1
    for m_, mt_, sx_ in ((None, mt, sx), (mask, mt, sx), (None, holes, neg), (mask, holes, neg)):
        got, c = nm.mosaic_adjust_sums_host(sx_, sy, rows, dx, dy, mt_, FW, FH, Ga, Gb, mask=m_)
        want, cw = R.sums(sx_, sy, rows, dx, dy, mt_, FW, FH, Ga, Gb, mask=m_)
        assert c == cw and np.array_equal(bits(got), bits(want)), (rows, np.abs(got - want).max())
        if m_ is None and mt_ is mt:
            assert c == rows
    far = Ga.copy()
    far[6] = -9.0                                          # denominators <= 0 on the right half: those rows drop out
    got, c = nm.mosaic_adjust_sums_host(sx, sy, rows, dx, dy, mt, FW, FH, far, Gb)
    want, cw = R.sums(sx, sy, rows, dx, dy, mt, FW, FH, far, Gb)
    assert c == cw and np.array_equal(bits(got), bits(want)) and (rows < 63 or 0 < c < rows)


def test_loop_of_12_frames_against_the_model(nm, loop):
    s = loop
    G, n, L = s["G"], s["n"], s["L"]
    close = s["H"][L - 1].reshape(3, 3)
    before = R.chain_to_maps(s["chain"])
    tabm = list(s["tab"]) + [list(s["mask"])]
    links = [(a, b) + R.inlier_points(tabm, l) for l, (a, b) in enumerate(zip(s["la"], s["lb"]))]
    model = R.model_f64(before, links, FW, FH)
    e0, g0 = R.corner_error(before, G, FW, FH), R.loop_gap(before, close, FW, FH)
    e1, g1 = R.corner_error(model, G, FW, FH), R.loop_gap(model, close, FW, FH)
    print("model: corner %.4f -> %.4f px, gap %.4f -> %.4f px" % (e0, e1, g0, g1))
    assert e1 < e0 and g1 < g0
    assert e1 <= CORNER_BAR and g1 <= GAP_BAR
    chain_out, fstat, rms, stats = adjust(nm, s, iterations=8)
    twin = R.chain_to_maps(chain_out)
    e2, g2, d = R.corner_error(twin, G, FW, FH), R.loop_gap(twin, close, FW, FH), R.corner_error(twin, model, FW, FH)
    print("twin: corner %.4f px, gap %.4f px, to the model %.2e px, stats %s" % (e2, g2, d, stats))
    for name, maps in (("before", before), ("twin", twin)):  # the shrink bias of the anchored cost
        r = R.footprint_scale(maps, G, FW, FH)[1:]
        print("%s: footprint scale against the truth, frames 1 .. 11: mean %.5f min %.5f max %.5f" % (name, r.mean(), r.min(), r.max()))
    assert e2 <= e1 + 2 * TWIN_TO_MODEL and g2 <= g1 + 4 * TWIN_TO_MODEL
    assert e2 < e0 and g2 < g0 and e2 <= CORNER_BAR and g2 <= GAP_BAR
    assert stats[7] == R.END_CONVERGED and stats[1] <= stats[0] and stats[3] == L and stats[4] == n - 1
    assert stats[2] == s["mask"].sum() and fstat.all() and (rms > 0).all()
    assert np.array_equal(bits(chain_out[0]), bits(s["chain"][0]))


@pytest.mark.parametrize("reason", ["iterations", "converged", "step", "no_link", "min_rows", "unusable", "singular",
                                    "rose_at_once", "rose_after_a_step"])
def test_end_reason_and_the_cost_never_rises(nm, loop, reason):
    s, L = loop, loop["L"]
    same = lambda a, b: np.array_equal(bits(a), bits(b))
    if reason in ("iterations", "converged", "step", "no_link", "min_rows"):
        kw = dict(iterations=dict(iterations=1), converged=dict(iterations=16), step=dict(max_step=1e-3),
                  no_link=dict(link_status=np.zeros(L, np.int32)), min_rows=dict(min_rows=301))[reason]
        chain_out, fstat, rms, st = adjust(nm, s, **kw)
        assert st[1] <= st[0]
        if reason == "iterations":
            assert st[7] == R.END_ITERATIONS and st[5] == 1
        elif reason == "converged":
            assert st[7] == R.END_CONVERGED and st[6] < 2.0 ** -7
        elif reason == "step":
            assert st[7] == R.END_STEP and st[5] == 0 and st[6] > 1e-3 and same(chain_out, s["chain"])
        else:                                               # no link with 301 contributing rows: the same end
            assert st[7] == R.END_NO_LINK and st[3] == 0 and (rms == 0).all() and same(chain_out, s["chain"]) and fstat.all()
    elif reason == "unusable":                              # the anchor does not participate
        dead = s["chain"].copy()
        dead[4] = 0
        out = adjust(nm, s, chain=dead, anchor=4)
        assert out[3][7] == R.END_UNUSABLE and same(out[0], dead) and out[1][4] == 0 and out[1].sum() == 11
    elif reason == "singular":
        # A detached component (frames 2, 3 hang on nothing that reaches the anchor) without damping: singular here, and
        # never a NaN. Which end a rank-deficient system takes depends on rounding (SINGULAR, or STEP when a pivot comes
        # out tiny and positive: include/nm_abi.h); this case gives SINGULAR. Either way no step is applied.
        tab = [[c[0], c[2]] for c in s["tab"]]
        out = adjust(nm, s, la=[0, 2], lb=[1, 3], tab=tab, chain=s["chain"][:4], mask=None, damping=0.0)
        assert out[3][7] == R.END_SINGULAR and out[3][5] == 0 and np.isfinite(out[3]).all() and np.isfinite(out[2]).all()
        assert same(out[0], s["chain"][:4])
        damped = adjust(nm, s, la=[0, 2], lb=[1, 3], tab=tab, chain=s["chain"][:4], mask=None, damping=1e-6, max_step=1e3)
        assert damped[3][7] != R.END_SINGULAR and damped[3][1] <= damped[3][0]
    else:       # the cost rises: at the first step (nothing stays applied), or after one good step (that one stays)
        seed, steps = (3, 0) if reason == "rose_at_once" else (18, 1)
        tab, chain = pair_case(seed)
        out = nm.mosaic_adjust_host([0], [1], *tab, chain, FW, FH, iterations=8, max_step=1e6, damping=0.0)
        assert out[3][7] == R.END_COST_ROSE and out[3][5] == steps and out[3][1] <= out[3][0], out[3]
        assert same(out[0][0], chain[0]) and same(out[0][1], chain[1]) == (steps == 0)
        if steps:
            few = nm.mosaic_adjust_host([0], [1], *tab, chain, FW, FH, iterations=1, max_step=1e6, damping=0.0)
            assert few[3][7] == R.END_ITERATIONS and all(same(a, b) for a, b in zip(out[:3], few[:3]))


def test_participation_duplicates_reversal_and_anchor(nm, loop):
    s, n, L = loop, loop["n"], loop["L"]
    base = adjust(nm, s, iterations=8)
    # frame 6 has a zero chain row (as after a broken link): it and its links are ignored, the others are adjusted
    broken = s["chain"].copy()
    broken[6] = 0
    out = adjust(nm, s, chain=broken, iterations=8)
    touching = [l for l in range(L) if 6 in (s["la"][l], s["lb"][l])]
    assert out[1].tolist() == [int(k != 6) for k in range(n)] and out[3][3] == L - len(touching) and out[3][4] == n - 2
    assert (out[2][touching] == 0).all() and np.array_equal(bits(out[0][6]), bits(broken[6])) and out[3][7] == R.END_CONVERGED
    keep = [l for l in range(L) if l not in touching]
    sub = adjust(nm, s, la=[s["la"][l] for l in keep], lb=[s["lb"][l] for l in keep], tab=[[c[l] for l in keep] for c in s["tab"]],
                 mask=s["mask"][keep], chain=broken, iterations=8)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((out[0], out[1], out[2][keep]), (sub[0], sub[1], sub[2])))
    # a link below min_rows is ignored: the same as a status-0 link
    thin = s["mask"].copy()
    thin[3, 7:] = 0
    status = np.ones(L, np.int32)
    status[3] = 0
    a, b = adjust(nm, s, mask=thin, iterations=8), adjust(nm, s, link_status=status, iterations=8)
    assert a[3][3] == L - 1 and np.array_equal(bits(a[0]), bits(b[0])) and a[2][3].tolist() == [0, 0]
    # a reversed link (src and dst swapped) gives the same cost and the same maps up to rounding; a duplicate counts twice
    rev = [list(c) for c in s["tab"]]
    l = 5
    sx, sy, m, dx, dy, mt = (c[l] for c in s["tab"])
    idx = np.nonzero(s["mask"][l, :m])[0]
    cap = len(sx)
    nsx, nsy, ndx, ndy = np.full(cap, -1, F32), np.zeros(cap, F32), np.zeros(cap, F32), np.zeros(cap, F32)
    nsx[:len(idx)], nsy[:len(idx)] = dx[mt[idx]], dy[mt[idx]]
    ndx[:len(idx)], ndy[:len(idx)] = sx[idx], sy[idx]
    nmt = np.full(cap, -1, np.int32)
    nmt[:len(idx)] = np.arange(len(idx))
    for c, v in zip(rev, (nsx, nsy, len(idx), ndx, ndy, nmt)):
        c[l] = v
    la, lb = list(s["la"]), list(s["lb"])
    la[l], lb[l] = lb[l], la[l]
    mrev = s["mask"].copy()
    mrev[l] = 0
    mrev[l, :len(idx)] = 1
    out = adjust(nm, s, la=la, lb=lb, tab=rev, mask=mrev, iterations=8)
    assert abs(out[3][0] - base[3][0]) < 1e-12 * base[3][0] and out[3][2] == base[3][2]
    assert R.corner_error(R.chain_to_maps(out[0]), R.chain_to_maps(base[0]), FW, FH) < 1e-4
    dup = adjust(nm, s, la=s["la"] + [s["la"][l]], lb=s["lb"] + [s["lb"][l]], tab=[list(c) + [c[l]] for c in s["tab"]],
                 mask=np.concatenate([s["mask"], s["mask"][l:l + 1]]), iterations=8)
    assert dup[3][3] == L + 1 and np.array_equal(bits(dup[2][l]), bits(dup[2][L])) and dup[3][0] > base[3][0]
    # another anchor: its row is kept bit for bit and the loop closes as well (the cost is measured in the anchor's mosaic
    # coordinates, so the maps relative to the anchor are not those of anchor 0 bit for bit or even to a tenth of a pixel)
    out = adjust(nm, s, anchor=7, iterations=8)
    assert np.array_equal(bits(out[0][7]), bits(s["chain"][7])) and not np.array_equal(bits(out[0][0]), bits(s["chain"][0]))
    close = s["H"][L - 1].reshape(3, 3)
    assert out[3][7] == R.END_CONVERGED and out[3][1] < out[3][0] and out[3][4] == n - 1
    assert R.loop_gap(R.chain_to_maps(out[0]), close, FW, FH) < R.loop_gap(R.chain_to_maps(s["chain"]), close, FW, FH)


def test_refusals(nm, loop):
    s = loop
    good = dict(iterations=5, min_rows=8, damping=1e-6, max_step=64.0, anchor=0)
    for bad in (dict(iterations=0), dict(iterations=17), dict(min_rows=3), dict(damping=-1.0), dict(damping=float("nan")),
                dict(damping=float("inf")), dict(max_step=0.0), dict(max_step=float("inf")), dict(anchor=-1), dict(anchor=12),
                dict(la=[0] + s["la"][1:], lb=[0] + s["lb"][1:]), dict(la=[12] + s["la"][1:]), dict(lb=[-1] + s["lb"][1:]),
                dict(la=[], lb=[], tab=[[] for _ in range(6)], mask=None), dict(chain=s["chain"][:1]),
                dict(tab=[c[:-1] for c in s["tab"]]), dict(mask=s["mask"][:, :-1]), dict(link_status=np.ones(3, np.int32))):
        with pytest.raises(nm.NmError):
            adjust(nm, s, **dict(good, **bad))
    # the C entry itself: ranges and null pointers, before anything is read
    import ctypes as C
    lib = nm.lib()
    n, L, cap = s["n"], s["L"], len(s["tab"][0][0])
    tabs = [[np.ascontiguousarray(v) for v in s["tab"][k]] for k in (0, 1, 3, 4, 5)]
    nA = np.array(s["tab"][2], np.int32)
    arr = lambda vs: (C.c_void_p * len(vs))(*[v.ctypes.data for v in vs])
    tb = dict(sx=arr(tabs[0]), sy=arr(tabs[1]), nA=arr([nA[k:k + 1] for k in range(L)]), dx=arr(tabs[2]), dy=arr(tabs[3]),
              mt=arr(tabs[4]))
    la, lb = (C.c_int * L)(*s["la"]), (C.c_int * L)(*s["lb"])
    out = [np.zeros((n, 9), F32), np.zeros(n, np.int32), np.zeros((L, 2)), np.zeros(8)]
    chain = np.ascontiguousarray(s["chain"])

    def call(**kw):
        a = dict(n=n, L=L, la=la, lb=lb, cap=cap, chain=chain.ctypes.data, anchor=0, fw=FW, fh=FH, it=5, rows=8, damp=1e-6,
                 step=64.0, o0=out[0].ctypes.data, o1=out[1].ctypes.data, o2=out[2].ctypes.data, o3=out[3].ctypes.data, **tb)
        a.update(kw)
        return lib.nm_mosaic_adjust_host_f32(a["n"], a["L"], a["la"], a["lb"], a["sx"], a["sy"], a["nA"], a["cap"], a["dx"],
                                             a["dy"], a["mt"], None, None, a["chain"], a["anchor"], a["fw"], a["fh"], a["it"],
                                             a["rows"], a["damp"], a["step"], a["o0"], a["o1"], a["o2"], a["o3"])

    assert call() == 0
    hole = arr(tabs[0])
    hole[L - 1] = None
    for kw in (dict(n=1), dict(n=65), dict(L=0), dict(L=257), dict(cap=0), dict(cap=1 << 22), dict(fw=0), dict(fh=32768),
               dict(it=0), dict(it=17), dict(rows=3), dict(damp=-1e-9), dict(step=0.0), dict(anchor=n), dict(la=None),
               dict(lb=None), dict(sx=None), dict(sy=None), dict(nA=None), dict(dx=None), dict(dy=None), dict(mt=None),
               dict(chain=None), dict(o0=None), dict(o1=None), dict(o2=None), dict(o3=None), dict(sx=hole)):
        assert call(**kw) == 1, kw                         # hipErrorInvalidValue
    assert lib.nm_mosaic_adjust_workspace_bytes(1, 1) == 0 and lib.nm_mosaic_adjust_workspace_bytes(2, 257) == 0
    assert lib.nm_mosaic_adjust_workspace_bytes(64, 256) > lib.nm_mosaic_adjust_workspace_bytes(2, 1) > 0


def test_place_equals_the_plans_records(nm, loop):
    s, n = loop, loop["n"]
    geo = (FW, FH, 2000, 1500, 700, 500)
    H = s["H"][:n - 1].copy()
    for status, Hk in ((None, H), (np.array([1] * 6 + [0] + [1] * 4, np.int32), H)):
        records, chain, extent = nm.mosaic_plan_host(Hk, status, *geo)
        got = nm.mosaic_place_host(chain, *geo)
        assert np.array_equal(bits(got[0]), bits(records)) and np.array_equal(bits(got[1]), bits(extent))
        assert records[:, 13].sum() == (n if status is None else 7)
    behind = H.copy()
    behind[2] = np.array([1, 0, 0, 0, 1, 0, 0.01, 0, 1], F32)       # frame 3 alone has corners behind the camera
    records, chain, extent = nm.mosaic_plan_host(behind, None, *geo)
    got = nm.mosaic_place_host(chain, *geo)
    assert records[3, 13] == 0 and np.array_equal(bits(got[0]), bits(records)) and np.array_equal(bits(got[1]), bits(extent))
    # a frame status other than 1, or a row that is not finite, gives a zero record
    records, chain, extent = nm.mosaic_plan_host(H, None, *geo)
    fs = np.ones(n, np.int32)
    fs[5] = 0
    nan = chain.copy()
    nan[8, 4] = np.nan
    got = nm.mosaic_place_host(nan, *geo, frame_status=fs)
    assert not got[0][5].any() and not got[0][8].any()
    rest = [k for k in range(n) if k not in (5, 8)]
    assert np.array_equal(bits(got[0][rest]), bits(records[rest]))
    for bad in (dict(fw=0), dict(cw=40000), dict(ox=1 << 20)):
        a = dict(fw=FW, fh=FH, cw=2000, ch=1500, ox=700, oy=500)
        a.update(bad)
        with pytest.raises(nm.NmError):
            nm.mosaic_place_host(chain, **a)
    assert nm.lib().nm_mosaic_place_host_f32(n, None, None, *geo, records.ctypes.data, None) == 1
    assert nm.lib().nm_mosaic_place_host_f32(n, chain.ctypes.data, None, *geo, None, None) == 1
    assert nm.lib().nm_mosaic_place_host_f32(65, chain.ctypes.data, None, *geo, records.ctypes.data, None) == 1
