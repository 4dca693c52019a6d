"""Host-side contract of the batched frame ingest (nm_frame_ingest_batch_f32) and the uchar4 map resample
(nm_resample_map_u8x4): refusal of every invalid argument before any device access (run in a child process that sees
no GPU), the Python wrappers' validation, the batch limit, and the oracle identity the GPU tests rest on (the oracle's
uchar4 sampling equals its per-channel scalar sampling truncated to uint8)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

HIP_ERROR_INVALID_VALUE = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# nm_frame_ingest_batch_f32: keyword overrides of a valid mapped call (n = 3, 64 x 48 frames, 40 x 30 output)
INGEST_CASES = [dict(n=0), dict(n=-1), dict(n=65), dict(fw=0), dict(fh=0), dict(cols=0), dict(rows=-2),
                dict(fw=32768), dict(fh=40000), dict(cols=32768), dict(rows=32768),
                dict(null="frames"), dict(null="gray"), dict(null_elem="frames"), dict(null_elem="gray"),
                dict(null_elem="frames", n=64), dict(null="map_x"), dict(null="map_y"),
                dict(identity=True, undist=True), dict(identity=True, cols=40, rows=48),
                dict(identity=True, cols=64, rows=30), dict(undist=True, null_elem="undistorted")]
RESAMPLE_CASES = [dict(tw=0), dict(th=0), dict(tw=-5), dict(th=-1, tw=-1)]


def _ingest_call(n=3, fw=64, fh=48, cols=40, rows=30, null=None, null_elem=None, identity=False, undist=False):
    fake = 0x1000
    nn = max(n, 1)
    arrays = {}
    for name in ("frames", "gray", "undistorted"):
        vals = [fake] * nn
        if null_elem == name:
            vals[-1] = None
        arrays[name] = (C.c_void_p * nn)(*vals)
    args = dict(map_x=None if identity else fake, map_y=None if identity else fake, **arrays)
    if not undist:
        args["undistorted"] = None
    if null:
        args[null] = None
    if identity and (cols, rows) == (40, 30):
        # identity mode: the output size defaults to the frame's, so that a case refuses only for what it names
        cols, rows = fw, fh
    return _lib.nm_frame_ingest_batch_f32(n, args["frames"], fw, fh, args["map_x"], args["map_y"], cols, rows,
                                          args["gray"], args["undistorted"], None)


def _resample_call(tw=64, th=48, cols=40, rows=30):
    fake = 0x1000
    return _lib.nm_resample_map_u8x4(fake, fake, tw, th, fake, fake, cols, rows, None)


_lib = None


def _child_main():
    """Runs every case and prints the statuses as JSON. Refuses (exit 3, no call made) if a GPU is visible."""
    import json
    import sys
    import torch
    if torch.cuda.device_count() != 0:
        sys.exit(3)
    import niftymatch_amd as nm
    global _lib
    _lib = nm.lib()
    out = dict(ingest=[_ingest_call(**kw) for kw in INGEST_CASES],
               resample=[_resample_call(**kw) for kw in RESAMPLE_CASES],
               # nothing to do: 0 without a launch
               resample_empty=[_resample_call(cols=0), _resample_call(rows=-3), _resample_call(tw=0, cols=0)],
               # valid arguments pass the checks and reach the launch, which fails for want of a device
               ingest_valid=[_ingest_call(n=64), _ingest_call(n=1, identity=True), _ingest_call(undist=True)])
    print(json.dumps(out))


@pytest.fixture(scope="module")
def statuses():
    """The calls run in a fresh child process with every GPU hidden, so that even an entry whose checks had regressed
    could only fail to launch, never dereference the fake addresses on a real device."""
    import json
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    path = [here, os.path.dirname(here)] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",
               PYTHONPATH=os.pathsep.join(path))
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + ["-c", "import test_ingest_host as t; t._child_main()"], env=env,
                       cwd=here, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def _ids(cases):
    return lambda i: "-".join("%s=%s" % kv for kv in cases[i].items())


@pytest.mark.parametrize("case", range(len(INGEST_CASES)), ids=_ids(INGEST_CASES))
def test_ingest_invalid_arguments_refused(statuses, case):
    assert statuses["ingest"][case] == HIP_ERROR_INVALID_VALUE, INGEST_CASES[case]


@pytest.mark.parametrize("case", range(len(RESAMPLE_CASES)), ids=_ids(RESAMPLE_CASES))
def test_resample_map_invalid_texture_refused(statuses, case):
    assert statuses["resample"][case] == HIP_ERROR_INVALID_VALUE, RESAMPLE_CASES[case]


def test_resample_map_empty_output_is_a_no_op(statuses):
    assert statuses["resample_empty"] == [0, 0, 0]


def test_valid_calls_pass_the_checks(statuses):
    """n = 64, identity mode and a gray + undistorted call are not refused: they reach the launch, which fails only
    because no device is visible (a launch error, not hipErrorInvalidValue)."""
    assert all(s not in (0, HIP_ERROR_INVALID_VALUE) for s in statuses["ingest_valid"]), statuses["ingest_valid"]


def test_batch_limit_is_64_everywhere(nm):
    """NM_INGEST_MAX_BATCH (include/nm_abi.h) = niftymatch_amd.INGEST_MAX_BATCH = the kernel's pointer tables."""
    hdr = int(re.search(r"#define NM_INGEST_MAX_BATCH (\d+)", open(os.path.join(ROOT, "include", "nm_abi.h")).read()).group(1))
    src = open(os.path.join(ROOT, "niftymatch_amd", "csrc", "nm_ingest.hip")).read()
    tables = re.findall(r"\*(frames|gray|undistorted)\[(\w+)\];", src)
    assert sorted(t[0] for t in tables) == ["frames", "gray", "undistorted"]
    assert {t[1] for t in tables} == {"NM_INGEST_MAX_BATCH"}
    assert hdr == nm.INGEST_MAX_BATCH == 64
    assert "nm_frame_ingest_batch_f32" in nm.ABI_SYMBOLS and "nm_resample_map_u8x4" in nm.ABI_SYMBOLS


def test_python_wrappers_validate_before_the_call(nm):
    import torch
    f = torch.zeros((12, 16, 4), dtype=torch.uint8)
    u, v = torch.zeros((10, 14)), torch.zeros((10, 14))
    cases = [
        (lambda: nm.ingest_batch([]), "frames"),
        (lambda: nm.ingest_batch([f] * 65), "frames"),
        (lambda: nm.ingest_batch([f] * 65, u, v), "frames"),
        (lambda: nm.ingest_batch([f.float()]), "uint8"),
        (lambda: nm.ingest_batch([f[..., :3].contiguous()]), "uint8"),
        (lambda: nm.ingest_batch([f, torch.zeros((12, 17, 4), dtype=torch.uint8)]), "one shape"),
        (lambda: nm.ingest_batch([f], u), "both"),
        (lambda: nm.ingest_batch([f], None, v), "both"),
        (lambda: nm.ingest_batch([f], undistorted=True), "need a map"),
        (lambda: nm.ingest_batch([f], u, v[:5]), "map"),
        (lambda: nm.ingest_batch([f], u.double(), v.double()), "map"),
        (lambda: nm.ingest_batch([f], u[0], v[0]), "map"),
        (lambda: nm.ingest_batch([f], torch.zeros((2, 32768)), torch.zeros((2, 32768))), "outside"),
        (lambda: nm.ingest_batch([f]), "current device"),             # host tensors: never computed on the CPU
        (lambda: nm.ingest_batch([f, f], u, v, undistorted=True), "current device"),
        (lambda: nm.resample_map_u8x4(f[..., 0], u, v), "uint8"),
        (lambda: nm.resample_map_u8x4(f.float(), u, v), "uint8"),
        (lambda: nm.resample_map_u8x4(f, u, v[:, :3]), "map"),
        (lambda: nm.resample_map_u8x4(f, u.to(torch.float16), v.to(torch.float16)), "map"),
        (lambda: nm.resample_map_u8x4(f, u, v), "current device"),
    ]
    for call, words in cases:
        with pytest.raises(nm.NmError, match=words):
            call()


# ---- the oracle identity: uchar4 sampling = per-channel scalar sampling, truncated ----

def _random_homography(rng, fw, fh, cols, rows):
    """A map from the output grid into the frame: scale, rotation, mild perspective and a shift that makes it leave
    the frame on some sides."""
    deg, s = rng.uniform(-30, 30), rng.uniform(0.6, 1.4) * max(fw / cols, fh / rows)
    c, sn = s * np.cos(np.radians(deg)), s * np.sin(np.radians(deg))
    return np.array([[c, -sn, rng.uniform(-0.3, 0.3) * fw], [sn, c, rng.uniform(-0.3, 0.3) * fh],
                     [rng.uniform(-1e-3, 1e-3), rng.uniform(-1e-3, 1e-3), 1.0]], np.float32)


@pytest.mark.parametrize("fw,fh,cols,rows", [(160, 120, 160, 120), (131, 97, 140, 90), (57, 33, 90, 71)])
@pytest.mark.parametrize("seed", range(3))
def test_oracle_u8x4_sampling_equals_per_channel_sampling(oracle, fw, fh, cols, rows, seed):
    """The oracle's resample_perspective fed its own returned map is its uchar4 sampling; each channel equals
    resample_undistort of that channel's plane (U8N) at the same map, truncated to uint8."""
    rng = np.random.default_rng(1000 * seed + fw + cols)
    tex = rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8)
    res, xp, yp = oracle.resample_perspective(tex, cols, rows, _random_homography(rng, fw, fh, cols, rows), inverse=False)
    for c in range(4):
        want = oracle.resample_undistort(np.ascontiguousarray(tex[..., c]), xp, yp)
        assert want.min() >= 0 and want.max() < 256
        assert np.array_equal(res[..., c], want.astype(np.uint8)), c
    inside = (xp >= -0.5) & (xp < fw - 0.5) & (yp >= -0.5) & (yp < fh - 0.5)
    assert inside.sum() > 0.2 * cols * rows and (~inside).any()


# ---- the end-to-end scene of test_gpu_ingest: its precondition, checked on the CPU ----

E2E_CAM = (560.0, 560.0, 320.0, 240.0)          # fx, fy, cx, cy: the centre of a 640 x 480 view
E2E_K1 = 0.12                                   # distort with +k1, undistort with -k1


def e2e_maps(oracle):
    """((u, v) of the k1 = +0.12 map that distorts a view, (u, v) of the k1 = -0.12 map the ingest undistorts with)."""
    from test_gpu_mosaic import VH, VW
    yy, xx = (a.astype(np.float32) for a in np.mgrid[0:VH, 0:VW])
    cam = np.array(E2E_CAM, np.float32)
    return tuple(oracle.undistort_map(xx, yy, cam, np.array([k1, 0, 0], np.float32)) for k1 in (E2E_K1, -E2E_K1))


def oracle_u8x4(oracle, frame, u, v):
    """The oracle's uchar4 sampling at a map, channel by channel (test_oracle_u8x4_sampling_equals_per_channel_sampling)."""
    return np.stack([oracle.resample_undistort(np.ascontiguousarray(frame[..., c]), u, v).astype(np.uint8)
                     for c in range(4)], -1)


def e2e_oracle_gray_and_mask(oracle, raws, um, vm):
    """The oracle's ingest of raw distorted frames (gray of the undistorted uchar4 frame) and the arena mask: the
    resample_mask of a ones plane at the undistortion map, as float."""
    from test_gpu_mosaic import VH, VW
    mask = oracle.resample_mask(np.ones((VH, VW), np.float32), um, vm, 0.5).astype(np.float32)
    return [oracle.grayscale(oracle_u8x4(oracle, r, um, vm)) for r in raws], mask


@pytest.mark.parametrize("seed", [3, 4])
def test_e2e_scene_gives_enough_true_matches_per_link(oracle, seed):
    """Status 1 in test_gpu_ingest's end-to-end test is a condition on its inputs: on the undistorted frames the oracle
    alone finds at least 1 000 matches per link k -> k+1 that land within 1.5 px of where the true view maps put them."""
    from test_gpu_mosaic import VH, VW, _scene, _view_maps
    (up, vp), (um, vm) = e2e_maps(oracle)
    scene = _scene(seed)
    maps = _view_maps()
    raws = [oracle_u8x4(oracle, oracle.resample_perspective(scene, VW, VH, np.linalg.inv(A).astype(np.float32),
                                                            inverse=True)[0], up, vp) for A in maps]
    grays, mask = e2e_oracle_gray_and_mask(oracle, raws, um, vm)
    assert (mask >= 1).sum() > 0.9 * VW * VH
    dets = [oracle.sift_detect_describe(g, 8192, mask=mask) for g in grays]
    good = []
    for k in range(7):
        a, b = dets[k], dets[k + 1]
        res = oracle.sift_matches(a["desc"], b["desc"], 0.8, want_distance=False)[0]
        i = np.nonzero(res >= 0)[0]
        T = np.linalg.inv(maps[k + 1]) @ maps[k]
        p = T @ np.stack([a["x"][i], a["y"][i], np.ones(len(i))]).astype(np.float64)
        d = np.hypot(p[0] / p[2] - b["x"][res[i]], p[1] / p[2] - b["y"][res[i]])
        good.append(int((d <= 1.5).sum()))
    print("seed", seed, "true matches per link", good)
    assert min(good) >= 1000, good
