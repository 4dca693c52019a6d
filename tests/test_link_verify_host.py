"""Link verification on the host (nm_link_verify_host_f32) against tests/link_verify_ref.py: the integer restatement bit for
bit, closed-form cases, one case per reason bit, refused arguments, and what the photometric gate is worth on the synthetic
mosaic views (the figures are recorded in DESIGN.md section 7, "Link verification")."""
import numpy as np
import pytest

import link_verify_ref as R

F32 = np.float32
FRAMES = [(64, 48), (67, 35), (131, 97)]
STRIDES = [1, 2, 3, 7, 64]           # 64 is larger than the two small frames' heights: L = 0 there
MAPS = {
    "identity": np.eye(3),
    "translation": [[1, 0, 3.3], [0, 1, -2.7], [0, 0, 1]],
    "homography": [[1.02, 0.03, 2.1], [-0.02, 0.98, 1.3], [1e-4, -2e-4, 1]],
    "outside": [[1, 0, 1000], [0, 1, 0], [0, 0, 1]],
}


def frame(seed, fw, fh):
    """A smooth-ish frame with texture, values inside [0, 255]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:fh, 0:fw]
    f = 120 + 60 * np.sin(xx / 5.0 + seed) * np.cos(yy / 7.0) + 40 * rng.random((fh, fw))
    return np.clip(f, 0, 255).astype(F32)


def disc(fw, fh):
    """The field of view of a fetoscope: a disc."""
    yy, xx = np.mgrid[0:fh, 0:fw]
    return ((xx - fw / 2) ** 2 + (yy - fh / 2) ** 2 < (0.45 * min(fw, fh)) ** 2).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def one(nm, A, B, H, **kw):
    """The host twin on one pair: (status, reason, stats[8], sums as Python ints)."""
    st, why, stats, sums = nm.link_verify_host([A], [B], np.asarray(H, F32).reshape(1, 9), want_sums=True, **kw)
    return int(st[0]), int(why[0]), stats[0], [int(v) for v in sums[0]]


@pytest.mark.parametrize("size", FRAMES)
@pytest.mark.parametrize("masked", [False, True])
def test_host_twin_equals_integer_restatement(nm, size, masked):
    """Sums, reason and status exactly; the eight stats bit for bit (the restatement's fused multiply-adds are exact, from
    Fractions, so no ulp allowance is needed)."""
    fw, fh = size
    A, B = frame(1, fw, fh), frame(2, fw, fh)
    mask = disc(fw, fh) if masked else None
    for name, H in MAPS.items():
        for stride in STRIDES:
            for gates in (dict(min_overlap=0.5, min_ncc=0.25), dict(min_overlap=0.98, min_ncc=0.6, max_area_ratio=1.02)):
                got = one(nm, A, B, H, mask=mask, stride=stride, **gates)
                want = R.verify_int(A, B, H, mask=mask, stride=stride, **gates)
                assert got[:2] == want[:2], (size, masked, name, stride, gates)
            what = (size, masked, name, stride)
            assert got[3] == want[3], what
            assert got[:2] == want[:2], what
            assert np.array_equal(bits(got[2]), bits(want[2])), what
            if stride > min(fw, fh):
                assert got[3] == [0] * 7 and got[1] & R.LOW_OVERLAP
            if name == "outside":
                assert got[3][1] == 0 and got[3][0] > 0 or stride > min(fw, fh)


def test_identity_on_equal_frames(nm):
    """Under the identity the taps of lattice pixel (x, y) are (x .. x + 1, y .. y + 1), so N = L exactly when the lattice
    stays off the last column and row: 67 x 35 at stride 3 (x <= 64, y <= 31) and 64 x 48 at stride 7 (x <= 59, y <= 38). At
    stride 1 the last column and row alone drop out."""
    for (fw, fh), stride in (((67, 35), 3), ((64, 48), 7)):
        A = frame(3, fw, fh)
        st, why, stats, sums = one(nm, A, A, np.eye(3), stride=stride, min_overlap=1.0, min_ncc=0.999)
        assert sums[0] == sums[1] == (fw // stride) * (fh // stride) and (st, why) == (1, 0)
        assert abs(stats[4] - 1) <= 2.0 ** -40 and abs(stats[5]) <= 2.0 ** -40 and abs(stats[3] - 1) <= 2.0 ** -50
        assert sums[2] == sums[3] and sums[4] == sums[5] == sums[6]
    A = frame(3, 64, 48)
    _, _, _, sums = one(nm, A, A, np.eye(3), stride=1)
    assert sums[0] == 64 * 48 and sums[1] == 63 * 47


def test_gain_and_bias_of_an_affine_brightness_change(nm):
    """B = 2 A + 10 with A in [20, 120] (so B stays inside [0, 255]) under the identity. Levels: qa = 16 a + da and
    qb = 16 b + db with |da|, |db| <= 1/2, so qb = 2 qa + 160 + e with |e| <= 3/2 per pixel. A least-squares slope over
    x = qa moves by at most max|e| * sum|x - mean| / sum (x - mean)^2 <= max|e| / sd(x) (Cauchy-Schwarz), and the intercept
    in gray values by at most max|e| / 16 plus the slope's error times mean_a."""
    fw, fh = 67, 35
    A = (20 + 100 * np.random.default_rng(5).random((fh, fw))).astype(F32)
    B = (2 * A + 10).astype(F32)
    _, _, stats, sums = one(nm, A, B, np.eye(3), stride=1)
    N, Sa, Saa = sums[1], sums[2], sums[4]
    sd_levels = np.sqrt(Saa / N - (Sa / N) ** 2)
    d_gain = 1.5 / sd_levels
    assert abs(stats[4] - 2) <= d_gain
    assert abs(stats[5] - 10) <= 1.5 / 16 + d_gain * stats[6]
    assert stats[3] > 0.999


def test_one_case_per_reason_bit(nm):
    fw, fh = 64, 48
    A = frame(7, fw, fh)
    I = np.eye(3)
    kw = dict(stride=3, min_overlap=0.5, min_ncc=0.5)
    assert one(nm, A, A, I, **kw)[:2] == (1, 0)
    # bit 1: status_in = 0; a NaN in H. Stats are zero.
    st, why, stats = nm.link_verify_host([A], [A], I.reshape(1, 9), status=[0], **kw)
    assert (st[0], why[0]) == (0, R.UNUSABLE) and not stats.any()
    Hn = I.copy()
    Hn[1, 1] = np.nan
    st, why, stats, _ = one(nm, A, A, Hn, **kw)
    assert (st, why) == (0, R.UNUSABLE) and not stats.any()
    # bit 2: inliers just below and at min_inliers
    for inl, want in ((11, R.FEW_INLIERS), (12, 0)):
        st, why, _ = nm.link_verify_host([A], [A], I.reshape(1, 9), inliers=[inl], min_inliers=12, **kw)
        assert (st[0], why[0]) == (int(want == 0), want)
    # bit 4: a reflected map (B is A mirrored, so the photometric gate passes)
    refl = np.array([[-1, 0, fw - 1], [0, 1, 0], [0, 0, 1]], float)
    got = one(nm, A, A[:, ::-1].copy(), refl, **kw)
    assert got[:2] == (0, R.BAD_GEOMETRY) and got[2][3] > 0.99
    # bit 4: a non-positive corner denominator (at corner (fw, 0): 1 - fw / 64 = 0); the lattice itself stays in front
    got = one(nm, A, A, [[1, 0, 0], [0, 1, 0], [-1.0 / fw, 0, 1]], stride=3, min_overlap=0, min_ncc=-1)
    assert got[:2] == (0, R.BAD_GEOMETRY)
    # bit 4: the area ratio just inside and just outside max_area_ratio (a zoom by sqrt(r) about the origin; the
    # photometric gate is switched off, the frames do not match under a zoom)
    for scale, want in ((1.99, 0), (2.01, R.BAD_GEOMETRY), (1 / 1.99, 0), (1 / 2.01, R.BAD_GEOMETRY)):
        got = one(nm, A, A, np.diag([scale, scale, 1.0]), stride=3, max_area_ratio=4.0, min_overlap=0, min_ncc=-1)
        assert got[1] == want, scale
    # bits 8 and 16 together: a map wholly outside B (ncc is 0 by definition there)
    assert one(nm, A, A, MAPS["outside"], **kw)[:2] == (0, R.LOW_OVERLAP | R.LOW_NCC)
    # bit 8 alone: half of A maps outside B; what is left matches
    shift = np.array([[1, 0, 33.0], [0, 1, 0], [0, 0, 1]])
    B = np.zeros_like(A)
    B[:, 33:] = A[:, :fw - 33]
    assert one(nm, A, B, shift, **kw)[:2] == (0, R.LOW_OVERLAP)
    # bit 16 alone: a flat frame has ncc = 0 by definition; an unrelated frame has a low one
    flat = np.full_like(A, 100)
    got = one(nm, flat, flat, I, **kw)
    assert got[:2] == (0, R.LOW_NCC) and got[2][3] == 0
    noise = (255 * np.random.default_rng(8).random((fh, fw))).astype(F32)
    assert one(nm, A, noise, I, **kw)[:2] == (0, R.LOW_NCC)


def test_nan_and_out_of_range_pixels(nm):
    """A bad pixel of A leaves L (and N); a bad tap of B leaves N alone, for each of the lattice pixels that read it."""
    fw, fh = 64, 48
    A = frame(9, fw, fh)
    I = np.eye(3)
    base = one(nm, A, A, I, stride=1)[3]
    for bad in (np.nan, -0.5, 255.5, np.inf):
        A2 = A.copy()
        A2[10, 20] = bad
        s = one(nm, A2, A, I, stride=1)[3]
        assert (s[0], s[1]) == (base[0] - 1, base[1] - 1), bad
        assert s == R.sums_int(A2, A, I, stride=1)
        B2 = A.copy()
        B2[10, 20] = bad
        s = one(nm, A, B2, I, stride=1)[3]
        assert (s[0], s[1]) == (base[0], base[1] - 4), bad       # taps of (19..20, 9..10)
        assert s == R.sums_int(A, B2, I, stride=1)


def test_refused_arguments(nm):
    import ctypes as C
    A = frame(1, 64, 48)
    ok = dict(stride=4, min_inliers=16, max_area_ratio=4.0, min_overlap=0.5, min_ncc=0.5)
    H = np.eye(3, dtype=F32).reshape(1, 9)
    bad = [dict(stride=0), dict(stride=65), dict(min_inliers=-1), dict(max_area_ratio=0.5), dict(max_area_ratio=np.nan),
           dict(max_area_ratio=np.inf), dict(min_overlap=np.nan), dict(min_ncc=np.inf)]
    for b in bad:
        with pytest.raises(nm.NmError):
            nm.link_verify_host([A], [A], H, **dict(ok, **b))
    with pytest.raises(nm.NmError):
        nm.link_verify_host([], [], H)
    with pytest.raises(nm.NmError):
        nm.link_verify_host([A] * 65, [A] * 65, np.tile(H, (65, 1)))
    with pytest.raises(nm.NmError):
        nm.link_verify_host([A], [A[:, :32]], H)
    with pytest.raises(nm.NmError):
        nm.link_verify_host([A], [A], np.eye(3, dtype=F32).reshape(1, 9)[:, :8])
    # the C entries themselves (host and device: the device entry refuses before it touches anything, so host pointers do)
    L = nm.lib()
    tab = (C.c_void_p * 1)(A.ctypes.data)
    nul = (C.c_void_p * 1)(None)
    st, why, stats = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(8)
    p = lambda a: a.ctypes.data

    def call(n=1, ta=tab, tb=tab, fw=64, fh=48, Hp=p(H), stride=4, mi=16, ar=4.0, mo=0.5, mn=0.5, so=p(st), wo=p(why),
             xo=p(stats), ws=p(stats)):
        host = L.nm_link_verify_host_f32(n, ta, tb, fw, fh, None, Hp, None, None, stride, mi, ar, mo, mn, so, wo, xo)
        if host == 0 and ws is not None:
            return host, None                 # accepted: the device entry would launch, and these are host pointers
        dev = L.nm_link_verify_batch_dev_f32(n, ta, tb, fw, fh, None, Hp, None, None, stride, mi, ar, mo, mn, so, wo, xo, ws,
                                             None)
        return host, dev
    assert call() == (0, None)
    refused = [dict(n=0), dict(n=65), dict(fw=0), dict(fw=32768), dict(fh=0), dict(fh=32768), dict(stride=0), dict(stride=65),
               dict(fw=32767, fh=32767, stride=1), dict(ar=float("nan")), dict(ar=0.99), dict(mo=float("inf")),
               dict(mn=float("nan")), dict(mi=-1), dict(ta=None), dict(tb=nul), dict(Hp=None), dict(so=None), dict(wo=None),
               dict(xo=None)]
    for r in refused:
        host, dev = call(**r)
        assert host != 0 and dev != 0, r
    assert call(ws=None)[1] != 0
    assert L.nm_link_verify_workspace_bytes(0) == 0 and L.nm_link_verify_workspace_bytes(65) == 0
    assert L.nm_link_verify_workspace_bytes(64) == 64 * L.nm_link_verify_workspace_bytes(1) > 0


# ---- what it is worth: the mosaic views of tests/test_gpu_mosaic.py, built here on the host ----

VW, VH, SCENE_W, SCENE_H = 640, 480, 1240, 600


def view_maps():
    """A_k: view-k pixel -> scene pixel (a panning, slightly rolling camera), as tests/test_gpu_mosaic.py has them."""
    maps = []
    for k in range(8):
        deg = 0.0 if k == 0 else 1.5 * np.sin(k)
        c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        maps.append(np.array([[c, -s, 40 + 70 * k], [s, c, 50 + 14 * (-1) ** k], [0, 0, 1]], np.float64))
    return maps


def scene_bgr(seed):
    import helpers
    g = np.clip(helpers.blurred_frame(seed, SCENE_W, SCENE_H, sigma=2.0) * 1.4, 0, 255).astype(np.uint8)
    return np.stack([g, np.roll(g, 3, 1), np.roll(g, 5, 0)], -1)


def gray_views(scene):
    """The views' gray planes: each BGR channel of the scene sampled bilinearly at A_k (x, y) (zero outside the scene),
    stored as a byte like the device's resample does, then 0.07 B + 0.72 G + 0.21 R in float32."""
    yy, xx = np.mgrid[0:VH, 0:VW].astype(np.float64)
    out = []
    for A in view_maps():
        sx, sy = A[0, 0] * xx + A[0, 1] * yy + A[0, 2], A[1, 0] * xx + A[1, 1] * yy + A[1, 2]
        i, j = np.floor(sx).astype(int), np.floor(sy).astype(int)
        fx, fy = (sx - i)[..., None], (sy - j)[..., None]
        pad = np.zeros((SCENE_H + 2, SCENE_W + 2, 3))
        pad[1:-1, 1:-1] = scene
        tap = lambda dj, di: pad[np.clip(j + dj + 1, 0, SCENE_H + 1), np.clip(i + di + 1, 0, SCENE_W + 1)]
        v = (1 - fx) * (1 - fy) * tap(0, 0) + fx * (1 - fy) * tap(0, 1) + (1 - fx) * fy * tap(1, 0) + fx * fy * tap(1, 1)
        v = np.floor(np.clip(v / 255.0 * 255.9999, 0, 255))
        out.append((0.07 * v[..., 0] + 0.72 * v[..., 1] + 0.21 * v[..., 2]).astype(F32))
    return out


def link_maps():
    """(true maps view k -> view k + 1, the wrong maps of each link: identity, the true map shifted by 20 px, the map of
    a neighbouring link: k + 1, and 5 for link 6 -- links of equal parity pan alike, link 0's map is within a pixel or two of
    link 6's and gives ncc 0.92 there, so it is no wrong map)"""
    A = view_maps()
    true = []
    for k in range(7):
        Ht = np.linalg.inv(A[k + 1]) @ A[k]
        true.append(Ht / Ht[2, 2])
    shift = np.array([[1, 0, 20.0], [0, 1, 0], [0, 0, 1]])
    wrong = [[np.eye(3), shift @ true[k], true[k + 1 if k < 6 else k - 1]] for k in range(7)]
    return true, wrong


# an overlap no honest neighbour link has: the true map shifted by half a frame's width, further along the pan
def far_maps(true):
    return [np.array([[1, 0, -VW / 2.0], [0, 1, 0], [0, 0, 1]]) @ Ht for Ht in true]


@pytest.fixture(scope="module")
def worth(oracle):
    views = gray_views(scene_bgr(90))
    true, wrong = link_maps()
    f = lambda k, H: R.model_f64(views[k], views[k + 1], H.astype(F32), stride=4)
    return dict(views=views, true=true, wrong=wrong, far=far_maps(true),
                m_true=[f(k, true[k]) for k in range(7)],
                m_wrong=[[f(k, H) for H in wrong[k]] for k in range(7)],
                m_far=[f(k, H) for k, H in enumerate(far_maps(true))])


def test_defaults_sit_midway_between_true_and_wrong_links(nm, worth):
    """The unquantised float64 model alone sets the defaults. ncc: midway between the lowest true link and the highest of
    the three wrong maps per link. overlap: those three do not separate in overlap (the identity has overlap 1 by
    construction, a shift by 20 px loses 3 %), so the wrong side is coarser: the true map shifted by half a frame."""
    t_ncc = [m["ncc"] for m in worth["m_true"]]
    w_ncc = [m["ncc"] for ms in worth["m_wrong"] for m in ms]
    t_ov = [m["overlap"] for m in worth["m_true"]]
    f_ov = [m["overlap"] for m in worth["m_far"]]
    print("ncc true %.5f .. %.5f wrong %.5f .. %.5f" % (min(t_ncc), max(t_ncc), min(w_ncc), max(w_ncc)))
    print("overlap true %.5f .. %.5f half-frame %.5f .. %.5f wrong %.5f .. %.5f" % (
        min(t_ov), max(t_ov), min(f_ov), max(f_ov), min(m["overlap"] for ms in worth["m_wrong"] for m in ms),
        max(m["overlap"] for ms in worth["m_wrong"] for m in ms)))
    assert max(w_ncc) < min(t_ncc) and max(f_ov) < min(t_ov)
    assert abs(nm.LINK_MIN_NCC - 0.5 * (min(t_ncc) + max(w_ncc))) < 0.005
    assert abs(nm.LINK_MIN_OVERLAP - 0.5 * (min(t_ov) + max(f_ov))) < 0.005


def test_defaults_pass_true_links_and_reject_wrong_ones(nm, worth):
    v = worth["views"]
    As, Bs = v[:7], v[1:]
    st, why, _ = nm.link_verify_host(As, Bs, np.array(worth["true"], F32).reshape(7, 9))
    assert (st == 1).all() and (why == 0).all()
    for c in range(3):
        st, why, _ = nm.link_verify_host(As, Bs, np.array([w[c] for w in worth["wrong"]], F32).reshape(7, 9))
        assert (st == 0).all() and ((why & R.LOW_NCC) != 0).all(), c
    st, why, _ = nm.link_verify_host(As, Bs, np.array(worth["far"], F32).reshape(7, 9))
    assert (st == 0).all() and ((why & R.LOW_OVERLAP) != 0).all()


# |ncc(integer restatement) - ncc(unquantised model)| measured on the 7 true and 21 wrong links above: at most 3.155e-5;
# twice that is allowed between the host twin and the model
NCC_ALLOWANCE = 6.31e-5


def test_host_twin_ncc_close_to_the_unquantised_model(nm, worth):
    v = worth["views"]
    worst_ref = worst_twin = 0.0
    for k in range(7):
        for H, m in zip([worth["true"][k]] + worth["wrong"][k], [worth["m_true"][k]] + worth["m_wrong"][k]):
            ref = R.finalize(R.sums_int(v[k], v[k + 1], H.astype(F32), stride=4))[3]
            twin = one(nm, v[k], v[k + 1], H, stride=4)[2][3]
            worst_ref, worst_twin = max(worst_ref, abs(ref - m["ncc"])), max(worst_twin, abs(twin - m["ncc"]))
    print("ncc: restatement - model %.3e, twin - model %.3e" % (worst_ref, worst_twin))
    assert worst_twin <= NCC_ALLOWANCE
