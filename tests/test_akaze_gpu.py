"""GPU: AKAZE feature extraction on the device (csrc/akaze.hip, sfmhip_akaze_extract) against the host extractor of
sfm_opencv_amd/host/sfm_akaze.hpp, which tests/host/akaze_ref.cpp lays open.

Exact where the arithmetic is plain IEEE float (scale space, kcontrast, maxima, suppression, sub-pixel fit, row order): the host's bytes.
Within a measured tolerance where libm and the device maths library differ (angle, descriptor bits).  The suppression kernel alone on lists
that images do not produce, against tests/akaze_suppress_ref.py.  Then the behaviour test of tests/test_features_cpu.py on the device
extractor, the budget / capacity / order rules, the path into the Hamming2 matcher without leaving the device, the block cache's error path
and the drivers' --akaze-device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import akaze_suppress_ref as sref
import oracle as orc
from sfm_opencv_amd import _lib, api, features_io
from test_akaze_cpu import build_akaze_ref, run_akaze_ref, texture

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "sfm_opencv_amd", "host")

# Angle and descriptor tolerances (test 4).  Measured on an MI355X against the host extractor over ALL rows of bgr161x243 and gray640x656
# (profiles/r17_time_akaze.log): the largest angle difference was ANGLE_MEASURED degrees, the largest Hamming distance of a row
# DESC_MEASURED bits, and SHARE_MEASURED of the rows had a non-zero distance.  The bounds are four times the measured values (the device
# maths library may move by an ulp between releases); the angle bound has a floor of one float ulp at 360 degrees (2^-15).
ANGLE_MEASURED, DESC_MEASURED, SHARE_MEASURED = 3.0517578125e-05, 0.0, 0.0
A_TOL, D_TOL = max(4 * ANGLE_MEASURED, 2.0 ** -15), 4 * DESC_MEASURED


def _warp(img, A, t):
    """out(p) = img(A^-1 (p - t)), bilinear; A 2x2, t 2"""
    h, w = img.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    Ai = np.linalg.inv(A)
    sx = Ai[0, 0] * (xx - t[0]) + Ai[0, 1] * (yy - t[1]); sy = Ai[1, 0] * (xx - t[0]) + Ai[1, 1] * (yy - t[1])
    x0 = np.clip(np.floor(sx).astype(int), 0, w - 2); y0 = np.clip(np.floor(sy).astype(int), 0, h - 2)
    fx = np.clip(sx - x0, 0, 1); fy = np.clip(sy - y0, 0, 1)
    out = (img[y0, x0] * (1 - fx) * (1 - fy) + img[y0, x0 + 1] * fx * (1 - fy) + img[y0 + 1, x0] * (1 - fx) * fy + img[y0 + 1, x0 + 1] * fx * fy)
    inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    return np.where(inside, out, 100.0)


def _bgr(gray, tint=(0.8, 0.9, 1.0)):
    g = np.clip(gray, 0, 255)
    return np.stack([g * tint[0], g * tint[1], g * tint[2]], 2).astype(np.uint8)


def _padded(img, pad):
    """the same image in a buffer whose rows are `pad` bytes longer than they need to be (filled with a value no pixel should see)"""
    rows, rowbytes = img.shape[0], img[0].size
    buf = np.full((rows, rowbytes + pad), 0xA5, np.uint8)
    buf[:, :rowbytes] = img.reshape(rows, rowbytes)
    return np.lib.stride_tricks.as_strided(buf, img.shape, (rowbytes + pad,) + img.strides[1:])


IMAGES = {
    "gray80x80": lambda: texture(80, 80, 7, blobs=300, smin=1.0, smax=3.0).astype(np.uint8),       # 4 levels; a 10 x 10 scan window on the first, none on the others
    "gray79x200": lambda: texture(79, 200, 2).astype(np.uint8),                                     # no level
    "bgr161x243": lambda: _bgr(texture(161, 243, 21)),                                              # 8 levels, odd half-sampling 161 -> 80, 243 -> 121
    "gray330x350": lambda: texture(330, 350, 3).astype(np.uint8),                                   # 12 levels
    "flat120x160": lambda: np.full((120, 160), 128, np.uint8),                                      # hmax == 0
    "gray640x656": lambda: texture(640, 656, 9, blobs=2800).astype(np.uint8),                       # 16 levels, the 29-step cycle
}
LEVELS = {"gray80x80": 4, "gray79x200": 0, "bgr161x243": 8, "gray330x350": 12, "flat120x160": 4, "gray640x656": 16}
TEXTURED = ["gray80x80", "bgr161x243", "gray330x350", "gray640x656"]
_images, _host = {}, {}


def image(name):
    if name not in _images:
        _images[name] = IMAGES[name]()
        _images[name].setflags(write=False)
    return _images[name]


def dev_image(name):
    return _padded(image(name), 5) if name == "bgr161x243" else image(name)


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    return build_akaze_ref(tmp_path_factory.mktemp("akaze_ref"))


@pytest.fixture
def host(ref_exe, tmp_path):
    """host(name, max_features=0): the host extractor's results on a named image, computed once per session"""
    def get(name, max_features=0):
        key = (name, max_features)
        if key not in _host:
            _host[key] = run_akaze_ref(ref_exe, image(name), str(tmp_path), max_features)
        return _host[key]
    return get


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. scale space
@pytest.mark.parametrize("name", list(IMAGES))
def test_scale_space_has_the_hosts_bytes(ctx, host, name):
    ref = host(name)
    img = dev_image(name)
    assert ref["n_levels"] == LEVELS[name] and ctx.akaze_levels(img) == ref["n_levels"]
    for lv in range(ref["n_levels"]):
        for kind, what in enumerate(("Lt", "Lsmooth", "Lx", "Ly", "Ldet")):
            got, n_levels, kc = ctx.akaze_scale_space(img, lv, kind)
            want = ref["levels"][lv][kind]
            assert n_levels == ref["n_levels"] and got.shape == want.shape
            assert np.array_equal(_bits(got), _bits(want)), (name, lv, what, np.abs(got - want).max(), (_bits(got) != _bits(want)).sum())
            assert _bits(kc) == _bits(ref["kc"][lv]), (name, lv, kc, ref["kc"][lv])
    if name == "flat120x160":
        assert ref["kc"][0] == np.float32(0.03)
    # a level that is not built is refused
    with pytest.raises(api.SfmHipError):
        ctx.akaze_scale_space(img, ref["n_levels"], 0)


# ------------------------------------------------------------------------------------------------ 2. suppression on lists
def _uniform_list(n, side, levels, seed):
    rng = np.random.default_rng(seed)
    level = np.sort(rng.integers(0, levels, n)).astype(np.int32)
    xyr = np.stack([rng.uniform(0, side, n), rng.uniform(0, side, n), rng.uniform(0.002, 1.0, n)], 1).astype(np.float32)
    return xyr, level


def _chain_list(n):
    """n points on a line, each within the radius (2.4 at level 0) of the one before, responses increasing: every candidate replaces the
    entry the one before it left, so each waits for its predecessor and a round resolves one of them"""
    xyr = np.stack([1.5 * np.arange(n), np.zeros(n), 0.01 + 0.001 * np.arange(n)], 1).astype(np.float32)
    return xyr, np.zeros(n, np.int32)


LISTS = {
    "n0": lambda: (np.zeros((0, 3), np.float32), np.zeros(0, np.int32)),
    "n1": lambda: _uniform_list(1, 30, 4, 1),
    "n64": lambda: _uniform_list(64, 30, 4, 2),
    "u300x30l4": lambda: _uniform_list(300, 30, 4, 3),
    "u300x30l8": lambda: _uniform_list(300, 30, 8, 4),
    "u1000x60l8": lambda: _uniform_list(1000, 60, 8, 5),
    "u3000x40l8": lambda: _uniform_list(3000, 40, 8, 6),
    "chain500": lambda: _chain_list(500),
}


@pytest.mark.parametrize("name", list(LISTS))
def test_suppression_on_lists_is_the_sequential_result(ctx, name):
    xyr, level = LISTS[name]()
    aux, want = sref.suppress(xyr, level)
    got = ctx.akaze_suppress(xyr, level)
    print("%s: %d candidates, %d in aux, %d kept" % (name, len(level), len(aux), len(want)))
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if name.startswith("u"):
        assert len(want) < len(aux) < len(level)          # not vacuous: replacements or drops in the first pass, drops in the second
    if name == "chain500":
        assert len(want) == 1 and want[0] == 499
    assert ctx.akaze_suppress(xyr, level).tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------ 3. extrema
@pytest.mark.parametrize("name", TEXTURED)
def test_extrema_stages_have_the_hosts_bits_and_order(ctx, host, name):
    ref = host(name)
    for stage in range(3):
        want_xysr, want_ol = ref["stages"][stage]
        xysr, ol = ctx.akaze_extrema(dev_image(name), stage)
        assert len(want_ol) > 0, "vacuous: the host finds nothing on this image"
        assert len(ol) == len(want_ol), (name, stage, len(ol), len(want_ol))
        assert np.array_equal(ol, want_ol), (name, stage)
        assert np.array_equal(_bits(xysr), _bits(want_xysr)), (name, stage, np.argwhere(_bits(xysr) != _bits(want_xysr))[:4])
    assert len(ref["stages"][1][1]) < len(ref["stages"][0][1]) or name == "gray80x80"


@pytest.mark.parametrize("name", ["gray79x200", "flat120x160"])
def test_images_without_key_points(ctx, name):
    kp, desc = ctx.akaze_extract(image(name))
    assert len(kp) == 0 and desc.shape == (0, 61) and desc.dtype == np.uint8
    for stage in range(3):
        assert len(ctx.akaze_extrema(image(name), stage)[1]) == 0


# ------------------------------------------------------------------------------------------------ 4. extract
def _extract_figures(ctx, host, name):
    ref = host(name)
    kp, desc = ctx.akaze_extract(dev_image(name))
    hk = ref["kp"]
    assert len(kp) == len(hk)
    for f in ("x", "y", "size", "response"):
        assert np.array_equal(_bits(kp[f]), _bits(hk[f])), f
    assert np.array_equal(kp["octave"], hk["octave"]) and np.array_equal(kp["class_id"], hk["class_id"])
    assert (desc[:, 60] >> 6 == 0).all()
    dang = np.abs((kp["angle"].astype(np.float64) - hk["angle"].astype(np.float64) + 540.0) % 360.0 - 180.0)
    ham = np.unpackbits(desc ^ ref["desc"], axis=1).sum(1)
    return dict(n=len(hk), dang=dang, ham=ham, kp=kp, desc=desc)


@pytest.mark.parametrize("name", ["gray80x80", "bgr161x243", "gray640x656"])
def test_extract_rows_are_the_hosts_and_angles_and_bits_within_the_measured_tolerance(ctx, host, name):
    f = _extract_figures(ctx, host, name)
    print("%s: %d rows; angle difference <= %.9g deg; Hamming distance per row <= %d bits, %.4f of the rows non-zero"
          % (name, f["n"], f["dang"].max(), f["ham"].max(), (f["ham"] > 0).mean()))
    assert f["n"] >= {"gray80x80": 1, "bgr161x243": 30}.get(name, 1000)          # not vacuous
    assert ANGLE_MEASURED <= 0.5 and DESC_MEASURED <= 8          # beyond that it is a bug to find, not a tolerance
    inside = (f["dang"] <= A_TOL) & (f["ham"] <= D_TOL)
    assert inside.mean() >= 0.99
    assert (f["kp"]["angle"] >= 0).all() and (f["kp"]["angle"] < 360.0001).all()


# ------------------------------------------------------------------------------------------------ 5. budget, capacity, order
def test_budget_capacity_order_and_repeatability(ctx, host):
    import torch
    name = "gray330x350"
    img = image(name)
    ref_all, ref_top = host(name), host(name, 40)
    k_all, d_all = ctx.akaze_extract(img)
    k_top, d_top = ctx.akaze_extract(img, max_features=40)
    assert len(ref_all["kp"]) > 100 and len(k_all) == len(ref_all["kp"])
    # the host's 40 rows: the head of the unbudgeted call, which is sorted on descending response
    assert len(k_top) == 40 and len(ref_top["kp"]) == 40
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        assert k_top[f].tobytes() == ref_top["kp"][f].tobytes(), f
    assert k_top.tobytes() == k_all[:40].tobytes() and d_top.tobytes() == d_all[:40].tobytes()
    assert (np.diff(k_all["response"]) <= 0).all()
    # a cap below the count: cap rows written, the full count reported, the rows behind them untouched
    cap = 30
    kp = np.zeros(cap + 3, api.KEYPOINT); desc = np.full((cap + 3, 61), 0xEE, np.uint8); n = C.c_int32(0)
    ctx._check(ctx.lib.sfmhip_akaze_extract(ctx.h, img.ctypes.data, img.shape[0], img.shape[1], 1, img.shape[1], 0, kp.ctypes.data, desc.ctypes.data, cap, C.byref(n)))
    assert n.value == len(k_all)
    assert kp[:cap].tobytes() == k_all[:cap].tobytes() and np.array_equal(desc[:cap], d_all[:cap])
    assert (desc[cap:] == 0xEE).all() and kp[cap:].tobytes() == bytes(3 * 28)
    # two runs: identical bytes
    k_again, d_again = ctx.akaze_extract(img)
    assert k_again.tobytes() == k_all.tobytes() and d_again.tobytes() == d_all.tobytes()
    # from a torch tensor, without leaving the device
    dev = torch.device("cuda", ctx.device)
    d_img = torch.from_numpy(np.array(img)).to(dev)
    cap = len(k_all) + 16
    d_kp = torch.zeros((cap, 28), dtype=torch.uint8, device=dev); d_desc = torch.zeros((cap, 61), dtype=torch.uint8, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    ctx.akaze_extract_dev(d_img, d_kp, d_desc, d_n)
    ctx.synchronize()
    assert int(d_n.item()) == len(k_all)
    assert d_kp[:len(k_all)].cpu().numpy().tobytes() == k_all.tobytes()
    assert d_desc[:len(k_all)].cpu().numpy().tobytes() == d_all.tobytes()


# ------------------------------------------------------------------------------------------------ 6. behaviour
def test_akaze_rows_and_hamming2_matching_under_a_similarity_on_the_device(ctx):
    """test_akaze_rows_and_hamming2_matching_under_a_similarity of tests/test_features_cpu.py with the device extractor and the Hamming2
    kernels, its thresholds unchanged"""
    img = texture(480, 640, 6)
    th = np.radians(-23.0); sc = 1.4
    A = sc * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]); t = np.array([-30.0, 140.0])
    tint = (0.8, 0.9, 1.0)          # BGR of the RGB tint (1.0, 0.9, 0.8) that test writes
    k1, d1 = ctx.akaze_extract(_bgr(img, tint))
    k2, d2 = ctx.akaze_extract(_bgr(_warp(img, A, t), tint))
    assert len(k1) > 150 and len(k2) > 100
    for d in (d1, d2):
        assert d.shape[1] == 61 and (d[:, 60] >> 6 == 0).all()
        ones = np.unpackbits(d, axis=1).sum(1)
        assert 150 < np.median(ones) < 340
    assert (k1["size"] > 2).all() and (k1["angle"] >= 0).all() and (k1["angle"] < 360).all() and (k1["response"] > 0.001).all()
    sets = [ctx.descset_hamming2(d1), ctx.descset_hamming2(d2)]
    m = ctx.match_pairs(sets, [[0, 1]])[0]
    for s in sets:
        s.close()
    assert np.array_equal(m, orc.match_features_hamming2(d1, d2))
    assert len(m) > 40
    p1 = np.stack([k1["x"][m["queryIdx"]], k1["y"][m["queryIdx"]]], 1); p2 = np.stack([k2["x"][m["trainIdx"]], k2["y"][m["trainIdx"]]], 1)
    err = np.linalg.norm(p1 @ A.T + t - p2, axis=1)
    assert (err < 2.5).mean() > 0.9 and np.median(err) < 1.0
    ok = err < 2.5
    ratio = k2["size"][m["trainIdx"]][ok] / k1["size"][m["queryIdx"]][ok]
    assert abs(np.median(ratio) - sc) < 0.25
    dang = (k2["angle"][m["trainIdx"]][ok] - k1["angle"][m["queryIdx"]][ok] + 540) % 360 - 180
    assert abs(abs(np.median(dang)) - 23.0) < 5.0


# ------------------------------------------------------------------------------------------------ 7. into the matcher
def test_rows_reach_the_matcher_without_leaving_the_device(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    img = texture(330, 350, 3)
    th = np.radians(5.0)
    A = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]); t = np.array([6.0, -4.0])
    imgs = [img.astype(np.uint8), _warp(img, A, t).astype(np.uint8)]
    sets, host_descs, keep = [], [], []
    for im in imgs:
        cap = 2048
        d_img = torch.from_numpy(im).to(dev)
        d_kp = torch.zeros((cap, 28), dtype=torch.uint8, device=dev); d_desc = torch.zeros((cap, 61), dtype=torch.uint8, device=dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
        ctx.akaze_extract_dev(d_img, d_kp, d_desc, d_n)
        ctx.synchronize()
        n = int(d_n.item())
        assert 100 < n <= cap
        s = ctx.descset_hamming2(d_desc[:n])
        assert s.info()["rows"] == n
        sets.append(s); host_descs.append(d_desc[:n].cpu().numpy()); keep.append((d_img, d_kp, d_desc))
        assert host_descs[-1].tobytes() == ctx.akaze_extract(im)[1].tobytes()          # the rows of the host-row path, byte for byte
    got = ctx.match_pairs(sets, [[0, 1]])[0]
    hsets = [ctx.descset_hamming2(d) for d in host_descs]
    want = ctx.match_pairs(hsets, [[0, 1]])[0]
    assert len(want) > 20 and got.tobytes() == want.tobytes()
    for s in sets + hsets:
        s.close()


# ------------------------------------------------------------------------------------------------ 8. block cache, driver
def test_a_failed_allocation_is_an_error_and_the_next_call_is_whole(ctx):
    img = image("bgr161x243")
    k0, d0 = ctx.akaze_extract(img)
    assert len(k0) > 10
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    try:
        kp = np.zeros(64, api.KEYPOINT); desc = np.zeros((64, 61), np.uint8); n = C.c_int32(0)
        rc = ctx.lib.sfmhip_akaze_extract(ctx.h, img.ctypes.data, img.shape[0], img.shape[1], 3, img.strides[0], 0, kp.ctypes.data, desc.ctypes.data, 64, C.byref(n))
        assert rc == _lib.E_HIP
    finally:
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 0) == 0
    k1, d1 = ctx.akaze_extract(img)
    assert k1.tobytes() == k0.tobytes() and d1.tobytes() == d0.tobytes()


def _write_ppm(path, bgr):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (bgr.shape[1], bgr.shape[0]))
        f.write(np.ascontiguousarray(bgr[:, :, ::-1]).tobytes())


def _scene_texture(h, w, seed):
    """the blobs of `texture`, each drawn inside four sigma of its centre (a 660 x 900 texture in a fraction of a second)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 110 + 20 * np.sin(xx / 97.0) + 15 * np.cos(yy / 71.0)
    for _ in range(int(700 * h * w / (360 * 480))):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        sg = rng.uniform(2.0, 9.0); a = rng.uniform(-70, 70)
        x0, x1 = max(int(cx - 4 * sg), 0), min(int(cx + 4 * sg) + 1, w); y0, y1 = max(int(cy - 4 * sg), 0), min(int(cy + 4 * sg) + 1, h)
        img[y0:y1, x0:x1] += a * np.exp(-((xx[y0:y1, x0:x1] - cx) ** 2 + (yy[y0:y1, x0:x1] - cy) ** 2) / (2 * sg * sg))
    return np.clip(img, 0, 255)


SCENE_F, SCENE_CX, SCENE_CY, SCENE_H, SCENE_W = 500.0, 240.0, 180.0, 360, 480
SCENE_CENTRES = [(0.0, 0.0), (0.6, 0.0), (1.2, 0.18)]          # cameras look along +z from (x, y, 0), no rotation


def _render_scene(tex, centre):
    """a textured relief Z(X, Y) = 10 + 0.8 sin(0.9 X) cos(0.7 Y) + 0.15 X (depth 8.3 to 12.5 over the views: real parallax, no plane) seen by a pinhole
    camera at (centre, 0) looking along +z: the depth along each pixel's ray by fixed-point iteration (the map contracts: |dZ/dd| <= 0.62 at
    the image corners), then the texture at the hit point, bilinear; the texture covers X in [-6, 9], Y in [-5.5, 5.5] at 60 pixels per unit"""
    v, u = np.mgrid[0:SCENE_H, 0:SCENE_W].astype(np.float64)
    dx, dy = (u - SCENE_CX) / SCENE_F, (v - SCENE_CY) / SCENE_F
    d = np.full_like(dx, 10.0)
    for _ in range(60):
        X, Y = centre[0] + d * dx, centre[1] + d * dy
        d = 10.0 + 0.8 * np.sin(0.9 * X) * np.cos(0.7 * Y) + 0.15 * X
    X, Y = centre[0] + d * dx, centre[1] + d * dy
    tx, ty = (X + 6.0) * 60.0, (Y + 5.5) * 60.0
    assert tx.min() >= 0 and ty.min() >= 0 and tx.max() <= tex.shape[1] - 2 and ty.max() <= tex.shape[0] - 2
    x0, y0 = np.floor(tx).astype(int), np.floor(ty).astype(int)
    fx, fy = tx - x0, ty - y0
    return tex[y0, x0] * (1 - fx) * (1 - fy) + tex[y0, x0 + 1] * fx * (1 - fy) + tex[y0 + 1, x0] * (1 - fx) * fy + tex[y0 + 1, x0 + 1] * fx * fy


def test_nview_driver_registers_three_views_with_the_device_extractor(ctx, ref_exe, tmp_path):
    """NViewReconstruct --akaze-device on three PPMs of a planted relief seen from three known camera centres, K.txt beside them: the counts
    it prints and the features it saves are the device extractor's, the third view is registered where it was planted, and without the
    flag the host extractor runs, byte for byte as before.

    The pose bounds.  The first pair fixes the scale (|T| = 1 between views 0 and 1), so the third centre is expected at (2, 0.3, 0) and
    its rotation at the identity.  Key points are located to about a pixel (the similarity test above: median below one pixel) at a focal
    length of 500 pixels, 0.1 degree per ray; with a baseline of 0.6 at depth 10 the triangulated depths, and a pose resected from
    them, carry about ten times that, a degree or two and a few percent of the baseline.  Bounds: 5 degrees on the rotation and on the
    direction of the centre, 25 % on its distance."""
    import re
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(HOST, "NViewReconstruct")
    tex = _scene_texture(660, 900, 41)
    imgs = [_bgr(_render_scene(tex, c)) for c in SCENE_CENTRES]
    d = tmp_path / "imgs"; d.mkdir()
    for i, im in enumerate(imgs):
        _write_ppm(d / ("%02d.ppm" % i), im)
    (d / "K.txt").write_text("%r %r %r %r\n" % (SCENE_F, SCENE_F, SCENE_CX, SCENE_CY))
    outs = {}
    for tag, extra in (("dev", ["--akaze-device"]), ("host", ["--features-only"]), ("host2", ["--features-only"])):
        feat = tmp_path / (tag + ".feat"); od = tmp_path / tag; od.mkdir()
        outs[tag] = (subprocess.run([exe, str(d), str(od), "--akaze"] + extra + ["--save-features=" + str(feat)], capture_output=True, text=True, check=True).stdout, feat)
    out = outs["dev"][0]
    fd = features_io.read_features(outs["dev"][1])
    assert len(fd["key_points"]) == 3
    for i, im in enumerate(imgs):
        kp, desc = ctx.akaze_extract(im)
        assert len(kp) > 100 and len(fd["key_points"][i]) == len(kp)
        assert fd["key_points"][i].tobytes() == kp.tobytes() and np.array_equal(fd["descriptors"][i], desc)
        assert ("%d 2D feature point detected." % len(kp)) in out          # the device extractor's counts
    assert out.count("Extracting features for image") == 3 and out.count("2D feature point detected.") == 3
    # registration: both later frames reconstructed, the cloud grows, the third view sits where it was planted
    assert "[Err]" not in out and "[Warning]" not in out
    assert "Frame 1 reconstructed." in out and "structure_ba.ply saved." in out
    total = int(re.search(r"Frame 1 point cloud fused, total (\d+) points now\.", out).group(1))
    assert total > 60
    head = out[:out.index("Frame 1 reconstructed.")]          # print_mat("R"), print_mat("T") of the frame: "R:\n[a, b, c;\n d, ...]\n"

    def last_mat(name, n):
        at = head.rindex(name + ":\n[") + len(name) + 3
        return np.array([float(v) for v in re.findall(r"[-+0-9.eE]+", head[at:head.index("]", at)])]).reshape(n)
    R, T = last_mat("R", (3, 3)), last_mat("T", (3,))
    c = -R.T @ T
    want = np.array([SCENE_CENTRES[2][0], SCENE_CENTRES[2][1], 0.0]) / SCENE_CENTRES[1][0]
    rot_deg = np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))
    dir_deg = np.degrees(np.arccos(np.clip(c @ want / (np.linalg.norm(c) * np.linalg.norm(want)), -1, 1)))
    print("third view: rotation %.3f deg from the identity, centre %s (planted %s): %.3f deg off, distance ratio %.4f; %d points"
          % (rot_deg, np.round(c, 4), np.round(want, 4), dir_deg, np.linalg.norm(c) / np.linalg.norm(want), total))
    assert rot_deg < 5.0 and dir_deg < 5.0 and abs(np.linalg.norm(c) / np.linalg.norm(want) - 1) < 0.25
    # without --akaze-device nothing changes: the host extractor, run to run the same file, and the rows of tests/host/akaze_ref.cpp
    assert open(outs["host"][1], "rb").read() == open(outs["host2"][1], "rb").read() and outs["host"][0] == outs["host2"][0]
    fh = features_io.read_features(outs["host"][1])
    for i in (0, 2):
        ref = run_akaze_ref(ref_exe, imgs[i], str(tmp_path))
        assert fh["key_points"][i].tobytes() == ref["kp"].tobytes() and np.array_equal(fh["descriptors"][i], ref["desc"])
