"""Obstacle grid and laser scan from the int32 map (sn_obstacles_from_raw, hobot_stereonet_amd/obstacles.py) without a GPU: the
numpy twin against an independent scalar loop written from the header's text (tests/golden/plain_refs.py), the beam table of the library against the
twin's, the struct in the header against its ctypes mirror, a known answer (a ground plane and a wall), and the parameter file."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from hobot_stereonet_amd import api, obstacles
from hobot_stereonet_amd.obstacles import ObstacleParams
from hobot_stereonet_amd.pointcloud import Camera
from plain_refs import obstacles_scalar_loop as _scalar_loop

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32
INT32_MIN = -(1 << 31)


def _maps_24x16(seed):
    """three maps of 24 x 16: random depths of 0.5 .. 6 m with zeros and negative words; a wall; a tilted plane"""
    rng = np.random.default_rng(seed)
    raw = np.empty((3, 16, 24), np.int32)
    raw[0] = rng.integers(800, 9600, (16, 24))
    raw[0][rng.random((16, 24)) < 0.15] = 0
    raw[0][rng.random((16, 24)) < 0.05] = -7
    raw[1] = 2400
    raw[2] = 1500 + 90 * np.arange(24)[None, :] + 40 * np.arange(16)[:, None]
    return raw


CASES = [
    (Camera(fx=20.0, fy=20.0, cx=11.5, cy=7.5, baseline_mm=120.0),
     ObstacleParams(base_from_cam=obstacles.mount(t=(0.0, 0.0, 0.4)), x_min_m=0.0, y_min_m=-2.0, cell_m=0.25, gw=24, gh=16, z_floor_m=-0.2,
                    z_lo_m=0.1, z_hi_m=1.2, min_obstacle_hits=2, min_ground_hits=1, beams=18, angle_min_rad=-0.72,
                    angle_increment_rad=0.08, range_min_m=0.3, range_max_m=5.0)),
    (Camera(fx=20.0, fy=22.0, cx=10.25, cy=6.0, baseline_mm=120.0, z_min_m=0.8, z_max_m=4.5, step=2),
     ObstacleParams(base_from_cam=obstacles.mount(0.3, 0.2, (0.1, -0.2, 0.6)), x_min_m=-0.5, y_min_m=-1.5, cell_m=0.3, gw=9, gh=11,
                    z_floor_m=-0.5, z_lo_m=0.0, z_hi_m=2.0, min_obstacle_hits=1, min_ground_hits=2, beams=40, angle_min_rad=-1.0,
                    angle_increment_rad=0.05, range_min_m=0.0, range_max_m=3.5)),
    (Camera(fx=20.0, fy=20.0, cx=11.5, cy=7.5, baseline_mm=120.0, step=4),
     ObstacleParams(x_min_m=0.0, y_min_m=-1.0, cell_m=0.5, gw=7, gh=4, z_floor_m=-1.0, z_lo_m=-0.1, z_hi_m=1.0, beams=0)),
    (Camera(fx=20.0, fy=20.0, cx=11.5, cy=7.5, baseline_mm=120.0),                        # yawed by 100 degrees: most of it behind
     ObstacleParams(base_from_cam=obstacles.mount(1.7453293, 0.0, (0.0, 0.0, 0.5)), gw=0, gh=0, z_floor_m=-0.3, z_lo_m=0.0, z_hi_m=2.0,
                    beams=16, angle_min_rad=-1.5, angle_increment_rad=0.18, range_min_m=0.0, range_max_m=50.0)),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_twin_equals_the_scalar_loop(case):
    cam, p = CASES[case]
    raw = _maps_24x16(case)
    edges = obstacles.beam_edges(p) if p.beams else None
    want = _scalar_loop(raw, cam.resolved(24, 16), p, edges)
    got = obstacles.reference(raw, cam, p)
    for name, g, w in zip(("occ", "hits", "height_mm", "ranges", "stats"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g.view(np.uint32) if g.dtype == f32 else g, w.view(np.uint32) if w.dtype == f32 else w), name
    occ, hits, height, ranges, stats = got
    if p.gw:
        assert hits.sum() > 0 and (height > INT32_MIN).any()
        assert np.array_equal(hits.sum(axis=(1, 2)), stats[:, :2])
    if p.beams:
        assert np.isfinite(ranges).any() and np.isinf(ranges).any()
    single = obstacles.reference(raw[1], cam, p)                   # a 2-D map drops the leading n
    assert all(np.array_equal(a, b[1], equal_nan=True) for a, b in zip(single, got))


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_beam_edges_of_the_library_and_the_twin():
    for beams, a0, da in ((31, -0.62, 0.04), (4096, -1.57, 3.14 / 4096), (1, 0.0, 1.5), (720, -1.5, 3.0 / 720), (7, 0.3, 0.01)):
        p = ObstacleParams(beams=beams, angle_min_rad=a0, angle_increment_rad=da)
        lib, twin = api.beam_edges(p), obstacles.beam_edges(p)
        assert lib.shape == twin.shape == (beams + 1,) and lib.dtype == f32
        assert _ulps(lib, twin).max() <= 1, (beams, a0, da)
        assert np.all(np.diff(lib) > 0)
        a = np.float64(f32(a0)) + np.arange(beams + 1) * np.float64(f32(da))
        assert np.allclose(lib, np.tan(a), rtol=1e-6)
    refused = {"no beams": (0, 0.0, 0.1), "too many": (4097, -1.0, 0.0004), "starts at -pi/2": (10, -1.5707964, 0.1),
               "ends beyond pi/2": (10, 0.0, 0.16), "ends on pi/2": (2, 0.0, 0.7853982), "decreasing": (10, 0.5, -0.05),
               "no increment": (10, 0.0, 0.0), "edges that do not differ": (8, 0.5, 1e-9), "nan": (4, float("nan"), 0.1),
               "inf": (4, 0.0, float("inf"))}
    for name, (beams, a0, da) in refused.items():
        p = ObstacleParams(beams=beams, angle_min_rad=a0, angle_increment_rad=da)
        with pytest.raises(ValueError):
            obstacles.beam_edges(p)
        with pytest.raises(api.StereoNetError) as e:
            api.beam_edges(p)
        assert e.value.code == -1, name
    lib = api.load_library()
    assert lib.sn_obstacle_beam_edges(None, np.zeros(4, f32).ctypes.data) == -1
    assert lib.sn_obstacle_beam_edges(C.byref(api.obstacle_params(ObstacleParams(beams=2, angle_increment_rad=0.1))), None) == -1


def test_header_struct_ctypes_mirror_and_abi_version_agree():
    src = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()
    assert re.search(r"#define SN_ABI_VERSION (\d+)", src).group(1) == "4" and api.ABI_VERSION == 4
    body = re.search(r"typedef struct sn_obstacle_params \{(.*?)\} sn_obstacle_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        if not words:
            continue
        for name in words[1:]:
            m = re.fullmatch(r"(\w+)\[(\d+)\]", name)
            fields.append((m.group(1), words[0], int(m.group(2))) if m else (name, words[0], 1))
    mirror = []
    for name, t in api.SnObstacleParams._fields_:
        count = getattr(t, "_length_", 1)
        base = getattr(t, "_type_", t) if count > 1 else t
        mirror.append((name, {C.c_float: "float", C.c_int: "int"}[base], count))
    assert fields == mirror
    assert C.sizeof(api.SnObstacleParams) == 4 * sum(c for _, _, c in fields) == 108
    # the dataclass carries every field of the struct (and the node's frame id)
    names = [f for f, _, _ in fields]
    assert names + ["frame"] == [f.name for f in __import__("dataclasses").fields(ObstacleParams)]
    lib = api.load_library()
    assert hasattr(lib, "sn_obstacles_from_raw") and hasattr(lib, "sn_obstacle_beam_edges")
    prm, cam = api.obstacle_params(ObstacleParams()), api.SnCamera(1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1)
    out = np.zeros(64, np.int32)
    assert lib.sn_obstacles_from_raw(None, 1, out.ctypes.data, C.byref(cam), C.byref(prm), None, out.ctypes.data, None, None, None, 0, None) == -1


W, H = 96, 64
KAT_CAM = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0)
KAT = ObstacleParams(base_from_cam=obstacles.mount(t=(0.0, 0.0, 0.5)), x_min_m=0.0, y_min_m=-2.0, cell_m=0.25, gw=20, gh=16, z_floor_m=-0.15,
                     z_lo_m=0.10, z_hi_m=1.5, min_obstacle_hits=3, min_ground_hits=3, beams=31, angle_min_rad=-0.62,
                     angle_increment_rad=0.04, range_min_m=0.0, range_max_m=10.0)


def test_known_answer_ground_plane_and_wall():
    """A level camera 0.5 m above the ground, a wall at Z = 3.1 m: one column of occupied cells at ix = 12, free cells where the
    ground rows reach, nothing known behind the wall; every range within 1 mm of the wall's distance along the beam's edges (half
    a step of the map, 2.5e-4 px, moves Z by Z^2 / (f B) * 2.5e-4 = 0.25 mm at 3.1 m)."""
    raw = obstacles.ground_and_wall(W, H, KAT_CAM, 0.5, 3.1)
    assert obstacles.mount(t=(0.0, 0.0, 0.5)) == (0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.5)
    occ, hits, height, ranges, stats = obstacles.reference(raw, KAT_CAM, KAT)
    assert occ.shape == (16, 20) and ranges.shape == (31,)
    iy, ix = np.nonzero(occ == 100)
    assert sorted(zip(iy.tolist(), ix.tolist())) == [(y, 12) for y in range(16)]
    assert np.all(occ[:, 13:] == -1) and np.all(hits[:, 13:] == 0)
    assert not np.any(occ[:, :12] == 100)
    free = 0
    for cy_ in range(16):
        for cx_ in range(12):
            corners = [(0.25 * (cx_ + a), -2.0 + 0.25 * (cy_ + b)) for a in (0, 1) for b in (0, 1)]
            if cx_ == 0:
                continue
            vs = [20.5 + 0.5 * 80.0 / x for x, _ in corners]
            us = [47.5 - 80.0 * y / x for x, y in corners]
            if min(vs) >= 34 and max(vs) <= 63 and min(us) >= 0 and max(us) <= 95:      # the cell lies within the ground rows' footprint
                assert occ[cy_, cx_] == 0, (cy_, cx_)
                free += 1
    assert free >= 20 and int(stats[3]) >= free and int(stats[2]) == 16
    assert np.array_equal(hits.sum(axis=(0, 1)), stats[:2])
    # the wall's top is the row v = 0: zb = 0.5 + 20.5 / 80 * 3.1 = 1.294 m
    assert np.all(np.abs(height[:, 12] - 1294) <= 2) and np.all(height[:, :12] == INT32_MIN)
    a = np.float64(f32(-0.62)) + np.arange(32) * np.float64(f32(0.04))
    finite = np.isfinite(ranges)
    assert not finite[[0, 1, 29, 30]].any() and finite[2:29].all()       # the image spans atan(47.5 / 80) = 0.536 rad to either side
    for b in np.nonzero(finite)[0]:
        near, far = sorted((abs(a[b]), abs(a[b + 1])))
        if a[b] < 0 < a[b + 1]:
            near = 0.0
        assert 3.1 / math.cos(near) - 1e-3 <= ranges[b] <= 3.1 / math.cos(far) + 1e-3, (b, float(ranges[b]))


def test_parameter_file_round_trip_and_errors(tmp_path):
    p = ObstacleParams(base_from_cam=obstacles.mount(0.1, 0.2, (0.3, 0.0, 0.45)), x_min_m=0.1, cell_m=0.05, gw=33, gh=44, beams=90,
                       angle_min_rad=-0.7, angle_increment_rad=0.7 / 45, range_min_m=0.2, range_max_m=8.0, frame="base_footprint")
    path = str(tmp_path / "ob.txt")
    obstacles.save_params(path, p)
    assert obstacles.load_params(path) == p
    with open(path, "w") as f:
        f.write("# only what differs from the defaults\ncell_m 0.2   # metres\nbeams 12\n")
    assert obstacles.load_params(path) == ObstacleParams(cell_m=0.2, beams=12)
    for text in ("cell 0.2\n", "cell_m 0.2 0.3\n", "gw ten\n", "beams 3\nbeams 4\n", "base_from_cam 1 2 3\n"):
        with open(path, "w") as f:
            f.write(text)
        with pytest.raises(ValueError):
            obstacles.load_params(path)
    for bad in (dict(cell_m=0.0), dict(gw=4097), dict(gw=0), dict(beams=-1), dict(z_lo_m=-1.0), dict(z_hi_m=0.0), dict(min_ground_hits=-1),
                dict(range_min_m=-0.1), dict(range_max_m=-1.0), dict(x_min_m=float("nan")), dict(base_from_cam=(float("inf"),) * 12)):
        assert obstacles.check(ObstacleParams(**bad)) is not None, bad
        with pytest.raises(ValueError):
            obstacles.reference(np.zeros((4, 4), np.int32), Camera(), ObstacleParams(**bad))
    assert obstacles.check(ObstacleParams()) is None
    img = obstacles.grid_image(np.array([[100, 0, -1], [0, 0, 0]], np.int8))       # [iy][ix] -> forward up, left to the left
    assert img.tolist() == [[255, 128], [255, 255], [255, 0]]
