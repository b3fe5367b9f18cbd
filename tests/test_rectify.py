"""Stereo rectification without a GPU: the library's map builder (sn_rectify_build_map, pure host) against the numpy twin
(hobot_stereonet_amd/rectify.py) word for word, the twin's Stage B on calibrations whose answer can be written down, the
geometry of stereo_rectify in float64, the calibration file's round trip and the binding against the header."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from hobot_stereonet_amd import api, rectify

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()


def _resize_only(sw, sh, w, h):
    e = rectify.Eye(0.9 * sw, 0.9 * sw, sw / 2 - 0.5, sh / 2 - 0.5)
    return rectify.Calib(sw, sh, e, e, 0.9 * sw * w / sw, 0.9 * sw * w / sw, (w - 1) / 2, (h - 1) / 2, 120.0)


# name -> (calibration, W, H, distorted)
@functools.lru_cache(maxsize=None)
def _cases():
    return {"identity": (rectify.identity(96, 64), 96, 64, False),
            "resize": (_resize_only(128, 80, 96, 64), 96, 64, False),
            "distorted-128x80": (rectify.synthetic_rig(128, 80, 96, 64, 128), 96, 64, True),
            "distorted-1920x1080": (rectify.synthetic_rig(1920, 1080, 1280, 720, 1920), 1280, 720, True),
            "behind": (rectify.behind_rig(128, 80, 96, 64), 96, 64, False)}


def check_nonvacuous(m, sw, sh, tag=""):
    """the conditions that keep a comparison on a distorted calibration's map from passing on nothing"""
    nv = rectify.nonvacuity(m, sw, sh)
    print(f"{tag}: {nv}")
    assert 0.01 < nv["sentinels"] < 0.50, nv
    assert nv["partly_outside"] >= 1, nv
    assert nv["both_fractions"] > 0.90, nv


@pytest.mark.parametrize("name", ["identity", "resize", "distorted-128x80", "distorted-1920x1080", "behind"])
def test_library_map_equals_twin_bit_for_bit(name):
    c, w, h, distorted = _cases()[name]
    for eye in (0, 1):
        want = rectify.build_map(c, eye, w, h)
        if distorted:
            check_nonvacuous(want, c.src_w, c.src_h, f"{name} eye {eye}")
        got = api.rectify_build_map(c, eye, w, h)
        diff = int((got != want).sum())
        print(f"{name} eye {eye}: {diff} differing words of {want.size}, {int(rectify.is_sentinel(want).sum())} sentinels")
        assert got.dtype == np.int32 and got.shape == (h, w, 2) and diff == 0
    if name == "identity":
        u, v = np.meshgrid(np.arange(w), np.arange(h))
        assert np.array_equal(want[..., 0], 256 * u) and np.array_equal(want[..., 1], 256 * v)
    if name == "behind":                                                          # part of the image lies behind the camera
        us, _ = rectify.map_point(c, 1, np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None])
        assert 0.1 < np.isnan(us).mean() < 0.9 and rectify.is_sentinel(want)[np.isnan(us)].all()
        assert not rectify.is_sentinel(want).all()


def test_build_map_argument_errors():
    lib = api.load_library()
    good = rectify.synthetic_rig(128, 80, 96, 64, 128)
    out = np.full((64, 96, 2), 7, np.int32)

    def rc(c, eye=0, w=96, h=64, o=out):
        return lib.sn_rectify_build_map(C.byref(api.stereo_calib(c)) if c is not None else None, eye, w, h,
                                        o.ctypes.data if o is not None else None)

    import dataclasses as dc
    bad = [dc.replace(good, left=dc.replace(good.left, d=(0.1, float("nan"), 0, 0, 0))),      # NaN in d
           dc.replace(good, right=dc.replace(good.right, d=(0.1, 0, 0, 0, float("inf")))),
           dc.replace(good, right=dc.replace(good.right, R=(float("nan"),) + good.right.R[1:])),
           dc.replace(good, pcx=float("nan")), dc.replace(good, pfx=0.0), dc.replace(good, pfy=-1.0),
           dc.replace(good, baseline_mm=0.0), dc.replace(good, left=dc.replace(good.left, fx=0.0)),
           dc.replace(good, right=dc.replace(good.right, fy=-2.0)), dc.replace(good, src_w=127), dc.replace(good, src_h=81),
           dc.replace(good, src_w=0), dc.replace(good, src_h=8194)]
    for c in bad:
        assert rc(c) == -1, c
        assert not c.ok()
        with pytest.raises(ValueError):
            rectify.build_map(c, 0, 96, 64)
    assert [rc(None), rc(good, o=None), rc(good, eye=2), rc(good, eye=-1), rc(good, w=0), rc(good, h=0)] == [-1] * 6
    assert np.all(out == 7)                                                       # no failed call wrote anything
    assert rc(good) == 0 and rc(dc.replace(good, src_w=8192, src_h=2)) == 0 and not np.all(out == 7)


def _frames(sw, sh, n, seed):
    """n random side-by-side NV12 frames of two sw x sh eyes: uint8 (n, sh * 3/2, 2 sw)"""
    return np.random.default_rng(seed).integers(0, 256, (n, sh + sh // 2, 2 * sw), dtype=np.uint8)


def test_twin_identity_returns_the_input_bytes():
    w, h = 96, 64
    f = _frames(w, h, 2, 1)
    assert np.array_equal(rectify.reference(rectify.identity(w, h), w, h, f, n=2), f)
    # separate eyes at a pitch of their own are the same call
    left, right = np.ascontiguousarray(f[:, :, :w]), np.ascontiguousarray(f[:, :, w:])
    assert np.array_equal(rectify.reference(rectify.identity(w, h), w, h, left, right, n=2), f)


def test_twin_integer_shift_moves_columns_and_fills_the_border():
    import dataclasses as dc
    w, h = 96, 64
    f = _frames(w, h, 1, 2)
    for k in (6, 5):
        got = rectify.reference(dc.replace(rectify.identity(w, h), pcx=float(k)), w, h, f)[0]
        for eye in (0, 1):
            src, out = f[0][:, eye * w:(eye + 1) * w], got[:, eye * w:(eye + 1) * w]
            assert np.array_equal(out[:h, k:], src[:h, :w - k]) and np.all(out[:h, :k] == 0)          # luma: Y = 0 in the vacated columns
            if k % 2 == 0:                                                                            # chroma: k/2 samples of two bytes
                assert np.array_equal(out[h:, k:], src[h:, :w - k]) and np.all(out[h:, :k] == 128)
            else:       # an odd shift is half a chroma sample: the mean of two neighbours, rounded up, per channel
                uv, suv = out[h:].reshape(h // 2, w // 2, 2).astype(int), src[h:].reshape(h // 2, w // 2, 2).astype(int)
                cj = np.arange(w // 2)
                first = (k + 1) // 2                                              # the first sample whose entry 2cj >= k has a source
                a, b = suv[:, cj[first:] - first], suv[:, cj[first:] - first + 1]
                assert np.array_equal(uv[:, first:], (a + b + 1) >> 1) and np.all(uv[:, :first] == 128)


def test_twin_half_pixel_shift_is_the_rounded_mean():
    import dataclasses as dc
    w, h = 96, 64
    f = _frames(w, h, 1, 3)
    got = rectify.reference(dc.replace(rectify.identity(w, h), pcx=0.5), w, h, f)[0]
    for eye in (0, 1):
        src = f[0][:h, eye * w:(eye + 1) * w].astype(int)
        a = np.concatenate([np.zeros((h, 1), int), src[:, :-1]], axis=1)           # the tap left of column 0 is the border, 0
        assert np.array_equal(got[:h, eye * w:(eye + 1) * w], (a + src + 1) >> 1)


def test_tensor_twin_equals_the_preprocess_golden(golden_pre):
    """rectify.tensor_from_sbs is the numpy form of sn_preprocess_sbs_nv12_batch; the golden vectors pin it to the reference"""
    for c in ("ramp8x4", "rand32x16", "rand64x36", "rand48x20"):
        w, h = map(int, golden_pre[c + ".wh"])
        eye = golden_pre[c + ".nv12"].reshape(h * 3 // 2, w)
        sbs = np.concatenate([eye, eye[::-1]], axis=1)[None]                      # the right eye: the same bytes, rows reversed
        got = rectify.tensor_from_sbs(sbs)[0].view(np.uint8) ^ np.uint8(0x80)
        assert np.array_equal(got[:3], golden_pre[c + ".yuv444"].reshape(3, h, w)), c
        assert np.array_equal(got[3], eye[::-1][:h]) and got.shape == (6, h, w)


def _project_raw(K, D, X):
    """a 3-D point in a raw camera's frame through its plumb-bob model -> pixel"""
    a, b = X[0] / X[2], X[1] / X[2]
    r2 = a * a + b * b
    k1, k2, p1, p2, k3 = D
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = a * rad + 2 * p1 * a * b + p2 * (r2 + 2 * a * a)
    yd = b * rad + p1 * (r2 + 2 * b * b) + 2 * p2 * a * b
    return K[0] * xd + K[2], K[1] * yd + K[3]


def test_stereo_rectify_geometry():
    worst = {"rows": 0.0, "disp": 0.0, "map": 0.0}
    for seed in range(4):
        c, K, D, R, T = rectify.synthetic_rig(640, 400, 480, 300, 40 + seed, zoom=1.0, with_extrinsics=True)
        R1, R2 = np.array(c.left.R).reshape(3, 3), np.array(c.right.R).reshape(3, 3)
        for Rk in (R1, R2):                                                       # proper rotations
            assert np.abs(Rk @ Rk.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Rk) - 1) < 1e-14
        assert c.baseline_mm == pytest.approx(np.linalg.norm(T), rel=1e-15) and c.pfx == c.pfy
        assert (c.pcx, c.pcy) == ((480 - 1) / 2, (300 - 1) / 2)
        rng = np.random.default_rng(seed)
        for _ in range(50):                                                       # 200 points over the four rigs
            X1 = np.array([rng.uniform(-600, 600), rng.uniform(-350, 350), rng.uniform(1500, 6000)])
            X2 = R @ X1 + T
            Xl, Xr = R1 @ X1, R2 @ X2
            ul, vl = c.pfx * Xl[0] / Xl[2] + c.pcx, c.pfy * Xl[1] / Xl[2] + c.pcy
            ur, vr = c.pfx * Xr[0] / Xr[2] + c.pcx, c.pfy * Xr[1] / Xr[2] + c.pcy
            worst["rows"] = max(worst["rows"], abs(vl - vr))
            want = c.pfx * np.linalg.norm(T) / Xl[2]
            worst["disp"] = max(worst["disp"], abs((ul - ur) - want) / want)
            for eye, (u, v, K_, D_, X) in enumerate(((ul, vl, K[0], D[0], X1), (ur, vr, K[1], D[1], X2))):
                us, vs = rectify.map_point(c, eye, u, v)
                pu, pv = _project_raw(K_, D_, X)
                worst["map"] = max(worst["map"], abs(float(us) - pu), abs(float(vs) - pv))
    print(worst)
    assert worst["rows"] <= 1e-9 and worst["disp"] <= 1e-9 and worst["map"] <= 1e-9
    # a rig that is rectified already stays as it is
    c = rectify.stereo_rectify((500, 500, 320, 200), None, (500, 500, 320, 200), None, np.eye(3), (-120.0, 0, 0), (640, 400), (640, 400))
    assert c.left.R == rectify.IDENTITY and c.right.R == rectify.IDENTITY and c.baseline_mm == 120.0 and c.pfx == 500.0
    with pytest.raises(ValueError):
        rectify.stereo_rectify((500, 500, 320, 200), None, (500, 500, 320, 200), None, np.eye(3), (120.0, 0, 0), (640, 400), (640, 400))
    with pytest.raises(ValueError):                                               # a rational model's extra coefficients
        rectify.stereo_rectify((500, 500, 320, 200), [0.1, 0, 0, 0, 0, 0.2], (500, 500, 320, 200), None, np.eye(3), (-120.0, 0, 0),
                               (640, 400), (640, 400))


def test_calibration_file_round_trip(tmp_path):
    for i, c in enumerate((rectify.synthetic_rig(1920, 1080, 1280, 720, 7), rectify.identity(96, 64), rectify.behind_rig(128, 80, 96, 64))):
        p = str(tmp_path / f"c{i}.txt")
        rectify.save_calib(p, c)
        assert rectify.load_calib(p) == c
    text = open(p).read()
    assert [ln.split()[0] for ln in text.splitlines() if not ln.startswith("#")] == list(rectify.KEYS)
    (tmp_path / "spaced.txt").write_text("# comment\n\n" + text.replace("P ", "  P   ") + "   # trailing\n")
    assert rectify.load_calib(str(tmp_path / "spaced.txt")) == c
    for broken in (text.replace("baseline_mm", "baseline"), text + "P 1 2 3 4\n", "\n".join(text.splitlines()[:-1]) + "\n",
                   text.replace("left.D", "left.D 0.5"), text.replace("size 128", "size 12x")):
        (tmp_path / "bad.txt").write_text(broken)
        with pytest.raises(ValueError):
            rectify.load_calib(str(tmp_path / "bad.txt"))


def test_rectify_binding_agrees_with_the_header():
    assert int(re.search(r"#define\s+SN_ABI_VERSION\s+(\d+)", HEADER).group(1)) == api.ABI_VERSION == 4      # purely additive
    ctype = {"double": C.c_double, "int": C.c_int, "uint32_t": C.c_uint32, "sn_eye_calib": api.SnEyeCalib}
    for name, struct in (("sn_eye_calib", api.SnEyeCalib), ("sn_stereo_calib", api.SnStereoCalib), ("sn_rectify_info", api.SnRectifyInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in (d.strip() for d in body.split(";") if d.strip()):
            t, names = decl.split(None, 1)
            for nm in (x.strip() for x in names.split(",")):
                m = re.fullmatch(r"(\w+)\[(\d+)\]", nm)
                fields.append((m.group(1), ctype[t] * int(m.group(2))) if m else (nm, ctype[t]))
        assert fields == list(struct._fields_), name
    assert C.sizeof(api.SnEyeCalib) == 18 * 8 and C.sizeof(api.SnStereoCalib) == 8 + 2 * 18 * 8 + 5 * 8
    assert "typedef struct sn_rectify sn_rectify;" in HEADER
    lib = api.load_library()
    protos = {
        "sn_rectify_build_map": (["const sn_stereo_calib *c", "int eye", "int w", "int h", "int32_t *map_xy"], C.c_int),
        "sn_rectify_create": (["sn_handle *h", "const sn_stereo_calib *c", "sn_rectify **out"], C.c_int),
        "sn_rectify_destroy": (["sn_rectify *r"], None),
        "sn_rectify_get_info": (["const sn_rectify *r", "sn_rectify_info *info"], C.c_int),
        "sn_rectify_get_camera": (["const sn_rectify *r", "sn_camera *cam"], C.c_int),
        "sn_rectify_get_map": (["sn_rectify *r", "int eye", "int32_t *map_xy_host"], C.c_int),
        "sn_rectify_nv12": (["sn_rectify *r", "int n", "const uint8_t *left", "const uint8_t *right", "int src_pitch",
                             "size_t src_frame", "uint8_t *out_sbs_nv12", "int8_t *out_nchw6", "int mem", "void *stream"], C.c_int)}
    special = {"const sn_stereo_calib *c": C.POINTER(api.SnStereoCalib), "sn_rectify **out": C.POINTER(C.c_void_p),
               "sn_rectify_info *info": C.POINTER(api.SnRectifyInfo), "sn_camera *cam": C.POINTER(api.SnCamera),
               "size_t src_frame": C.c_size_t}
    for name, (params, restype) in protos.items():
        ret = "void" if restype is None else "int"
        proto = re.search(r"\b%s\s+%s\((.*?)\);" % (ret, name), HEADER, re.S).group(1)
        assert [" ".join(t.split()) for t in proto.split(",")] == params, name
        fn = getattr(lib, name)
        assert fn.restype is restype and len(fn.argtypes) == len(params), name
        for at, prm in zip(fn.argtypes, params):
            assert at is (special[prm] if prm in special else C.c_int if prm.startswith("int ") else C.c_void_p), (name, prm)
    # the header carries the contract: Stage A's operations in their order, and Stage B's blend
    for line in ("X = R[0]*x + R[3]*y + R[6];  Y = R[1]*x + R[4]*y + R[7];  Wc = R[2]*x + R[5]*y + R[8]",
                 "rad = 1.0 + r2*(k1 + r2*(k2 + r2*k3))", "mx = (int32)floor(us*256.0 + 0.5);  my = (int32)floor(vs*256.0 + 0.5)",
                 "out = ((256-fx)*(256-fy)*p(0,0) + fx*(256-fy)*p(1,0) + (256-fx)*fy*p(0,1) + fx*fy*p(1,1) + 32768) >> 16"):
        assert line in HEADER, line
    assert all(callable(getattr(api.Rectifier, f)) for f in ("rectify", "rectify_device", "map", "close"))
    assert callable(api.StereoNetHIP.rectifier) and rectify.SENTINEL == -2 ** 31


def test_compat_builds_the_rectify_harness():
    import subprocess
    from hobot_stereonet_amd import build
    build.build()
    compat = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
    subprocess.check_call(["make", "-C", compat, "-s"])
    assert os.path.exists(os.path.join(compat, "build", "rectify_harness"))
    src = open(os.path.join(compat, "src", "stereonet_node.cpp")).read()
    assert "STEREONET_RECTIFY" in src and "sn_rectify_nv12" in src
