"""Point cloud from the int32 map (sn_pointcloud_from_raw, hobot_stereonet_amd/pointcloud.py) without a GPU: the entry point
is exported and rejects bad arguments before touching a device, the numpy twin's known answers, PLY output, and the host
mirror (PointCloud2 stand-in, point-cloud harness) builds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hobot_stereonet_amd import api, pointcloud, spec
from hobot_stereonet_amd.pointcloud import COMPACT, ORGANISED, Camera

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMPAT = os.path.join(ROOT, "hobot_stereonet_amd", "csrc", "compat")
W, H = 96, 64


def _call(h, n=1, raw=True, cam=None, layout=ORGANISED, points=True, counts=True, nv12=None, pitch=0, mem=0):
    lib = api.load_library()
    r = np.zeros((n, H, W), np.int32)
    pts = np.zeros(n * H * W * 4 + 4, np.float32)
    p = pts.ctypes.data + (-pts.ctypes.data % 16)
    cnt = np.zeros(n, np.uint32)
    c = cam if cam is not None else api.SnCamera(1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1)
    return lib.sn_pointcloud_from_raw(h, n, r.ctypes.data if raw else None, nv12, pitch, C.byref(c), layout,
                                      p if points else None, cnt.ctypes.data if counts else None, mem, None)


def test_pointcloud_entry_point_exported_and_rejects_bad_arguments():
    lib = api.load_library()
    assert hasattr(lib, "sn_pointcloud_from_raw")
    assert _call(None) == -1                                      # NULL handle
    assert _call(None, layout=7) == -1                            # unknown layout
    assert _call(None, cam=api.SnCamera(1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 3)) == -1      # step 3
    assert _call(None, cam=api.SnCamera(0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1)) == -1      # fx <= 0
    assert _call(None, layout=COMPACT, counts=False) == -1       # compact needs counts
    assert _call(None, raw=False) == -1


def _raw_kat():
    raw = np.zeros((H, W), np.int32)
    raw[H // 2, W // 2] = 200000
    return raw


def test_twin_kat_principal_point_and_invalid_nan_pattern():
    """raw 200000 at (cx, cy) -> Z = 0.632 m, X = Y = 0; raw 0 is invalid: NaN x 3, rgb 0 as bits."""
    pts, cnt = pointcloud.reference(_raw_kat(), Camera())
    assert pts.shape == (H, W, 4) and cnt.tolist() == [1]
    x, y, z, _ = pts[H // 2, W // 2]
    assert x == 0.0 and y == 0.0 and abs(float(z) - 0.632) < 1e-3
    bits = pts.view(np.uint32)
    assert (bits[0, 0] == [0x7fc00000, 0x7fc00000, 0x7fc00000, 0]).all()
    assert (bits[..., :3] == 0x7fc00000).sum() == 3 * (H * W - 1)
    # the same depth as sn_depth_from_raw's host twin (Parse's float / double mix)
    f, b = np.float32(pointcloud.FOCAL), np.float32(pointcloud.BASELINE_MM)
    dis = np.float32(200000) * np.float32(spec.OUT_SCALE)
    assert z == np.float32(np.float64(f * b) / (np.float64(dis) * 16.0 * 12.0) / 1000.0)
    # compact: the one point, raster order
    cp, cc = pointcloud.reference(_raw_kat(), Camera(), COMPACT)
    assert cc.tolist() == [1] and np.array_equal(cp[0].view(np.uint32), pts[H // 2, W // 2].view(np.uint32))


def test_twin_xy_and_z_range_clipping():
    rng = np.random.default_rng(1)
    raw = rng.integers(-5, 400000, (2, H, W)).astype(np.int32)
    cam = Camera(fx=500.0, fy=480.0, cx=40.5, cy=30.25, z_min_m=0.6, z_max_m=1.2)
    pts, cnt = pointcloud.reference(raw, cam)
    full, _ = pointcloud.reference(raw, Camera(fx=500.0, fy=480.0, cx=40.5, cy=30.25))
    z = full[..., 2]
    want = (raw > 0) & (z >= np.float32(0.6)) & (z <= np.float32(1.2))
    assert 0 < want.sum() < (raw > 0).sum()
    assert np.array_equal(np.isfinite(pts[..., 2]), want) and cnt.tolist() == want.reshape(2, -1).sum(1).tolist()
    k, i, j = np.argwhere(want)[0]
    assert pts[k, i, j, 0] == np.float32((np.float32(j) - np.float32(40.5)) * pts[k, i, j, 2]) / np.float32(500.0)
    assert pts[k, i, j, 1] == np.float32((np.float32(i) - np.float32(30.25)) * pts[k, i, j, 2]) / np.float32(480.0)
    # no upper bound when z_max_m <= 0
    _, c0 = pointcloud.reference(raw, Camera(z_min_m=0.0, z_max_m=-1.0))
    assert c0.tolist() == (raw > 0).reshape(2, -1).sum(1).tolist()


@pytest.mark.parametrize("step", [2, 4])
def test_twin_step_shapes_odd_geometry(step):
    w, h = 97, 63
    rng = np.random.default_rng(step)
    raw = rng.integers(0, 400000, (h, w)).astype(np.int32)
    cam = Camera(step=step)
    pts, _ = pointcloud.reference(raw, cam)
    ho, wo = -(-h // step), -(-w // step)
    assert pts.shape == (ho, wo, 4) and cam.out_shape(w, h) == (ho, wo)
    full, _ = pointcloud.reference(raw, Camera())
    assert np.array_equal(pts.view(np.uint32), full[::step, ::step].view(np.uint32))
    cp, cc = pointcloud.reference(raw, cam, COMPACT)
    assert cp.shape == (ho * wo, 4)
    assert np.array_equal(cp[:cc[0]].view(np.uint32), pts[np.isfinite(pts[..., 2])].view(np.uint32))


def test_rgb_formula_cube_corners_and_grey_ramp():
    y, u, v = (a.ravel() for a in np.meshgrid([0, 255], [0, 255], [0, 255], indexing="ij"))
    got = pointcloud.nv12_to_rgb(y, u, v)
    uc, vc = u - 128, v - 128
    fix = lambda c: np.clip(np.floor(y + c + 0.5), 0, 255).astype(np.uint32)      # noqa: E731
    want = (fix(91881 / 65536 * vc) << 16) | (fix((-22554 * uc - 46802 * vc) / 65536) << 8) | fix(116130 / 65536 * uc)
    assert np.array_equal(got, want)
    assert got[0] == 0x008700 and got[-1] == 0xff79ff       # (0,0,0) -> (0,135,0); (255,255,255) -> (255,121,255)
    # within one level of the textbook JFIF coefficients
    text = np.stack([y + 1.402 * vc, y - 0.344136 * uc - 0.714136 * vc, y + 1.772 * uc], -1)
    text = np.clip(np.rint(text), 0, 255)
    rgb = np.stack([(got >> 16) & 255, (got >> 8) & 255, got & 255], -1)
    assert np.abs(rgb - text).max() <= 1
    ramp = np.arange(256)
    g = pointcloud.nv12_to_rgb(ramp, np.full(256, 128), np.full(256, 128))
    assert np.array_equal(g, (ramp << 16 | ramp << 8 | ramp).astype(np.uint32))


@pytest.mark.parametrize("pitch_mult", [1, 2])
def test_twin_colour_sampling_true_nv12(pitch_mult):
    """Y at (v, u); U, V at uv[(v>>1)*pitch + (u&~1)] / +1 of the frame's chroma plane; the side-by-side frame's left eye
    is the left half of every row (pitch 2W)."""
    w, h = 10, 6
    pitch = pitch_mult * w
    rng = np.random.default_rng(pitch)
    frame = rng.integers(0, 256, pointcloud.nv12_frame_bytes(pitch, h), dtype=np.uint8)
    raw = np.full((h, w), 150000, np.int32)
    pts, _ = pointcloud.reference(raw, Camera(), nv12=frame, pitch=pitch)
    rgb = pts[..., 3].view(np.uint32)
    for v, u in ((0, 0), (3, 5), (5, 9), (4, 2)):
        uv = pitch * h + (v >> 1) * pitch + (u & ~1)
        assert rgb[v, u] == pointcloud.nv12_to_rgb(frame[v * pitch + u], frame[uv], frame[uv + 1])
    un = pointcloud.unpack_rgb(pts)
    assert un.shape == (h, w, 3) and un.dtype == np.uint8
    assert int(un[3, 5, 0]) == int(rgb[3, 5]) >> 16
    # no colour: the 4th word is 0
    p0, _ = pointcloud.reference(raw, Camera())
    assert (p0[..., 3].view(np.uint32) == 0).all()


def test_write_ply_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 400000, (H, W)).astype(np.int32)
    frame = rng.integers(0, 256, pointcloud.nv12_frame_bytes(W, H), dtype=np.uint8)
    pts, cnt = pointcloud.reference(raw, Camera(), COMPACT, nv12=frame, pitch=W)
    path = str(tmp_path / "c.ply")
    assert pointcloud.write_ply(path, pts, int(cnt[0])) == cnt[0]
    assert open(path, "rb").read(3) == b"ply"
    v = pointcloud.read_ply(path)
    assert len(v) == cnt[0]
    for i, name in enumerate("xyz"):
        assert np.array_equal(v[name], pts[:cnt[0], i])
    rgb = pointcloud.unpack_rgb(pts[:cnt[0]])
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], -1), rgb)
    # an organised cloud: only its valid (finite) points are written
    org, oc = pointcloud.reference(raw, Camera(), nv12=frame, pitch=W)
    assert pointcloud.write_ply(str(tmp_path / "o.ply"), org) == oc[0]
    assert np.array_equal(pointcloud.read_ply(str(tmp_path / "o.ply"))["z"], v["z"])


def test_compat_builds_with_pointcloud2_stub():
    from hobot_stereonet_amd import build
    build.build()
    subprocess.check_call(["make", "-C", COMPAT, "-s"])
    assert os.path.exists(os.path.join(COMPAT, "build", "pointcloud_harness"))
