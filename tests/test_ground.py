"""The ground stage without a device: the numpy twin of sn_ground_from_raw against a plain loop over Python integers written
from the header's text (on small maps, and on maps at the declared limits, where the loop cannot overflow and the twin's int64
must not), the structs in the header against their ctypes mirrors, the gate, the parameter file, and geometric truth: seeded
scenes whose floor the fit must find to 0.5 % of the height and 0.1 degree of the normal."""
import ctypes as C
import dataclasses
import math
import os
import re

import numpy as np
import pytest

from hobot_stereonet_amd import api, ground, obstacles
from hobot_stereonet_amd.ground import GroundParams
from hobot_stereonet_amd.pointcloud import Camera

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32
SMALL = Camera(fx=16.0, fy=16.0, cx=12.0, cy=8.0, baseline_mm=120.0)          # 24 x 16
CAM = Camera(fx=64.0, fy=64.0, cx=48.0, cy=32.0, baseline_mm=120.0)           # 96 x 64


def _small_cases():
    """name -> (maps int32 (n, 16, 24), camera, parameters): every path of the contract at a size the plain loop takes in a second"""
    rng = np.random.default_rng(11)
    base = GroundParams(hypotheses=48, refits=2, tol_px=0.05, min_inliers=20, min_area=4, height_min_m=0.2, height_max_m=2.0)
    scenes = np.stack([ground.scene(24, 16, SMALL, 0.5, 0.1, 0.05, wall_z_m=4.0, hole_frac=0.1, outlier_frac=0.1, seed=3)[0],
                       ground.scene(24, 16, SMALL, 0.8, 0.0, 0.0, seed=4)[0],
                       ground.scene(24, 16, SMALL, 0.4, 0.3, -0.1, wall_z_m=1.2, boxes=1, seed=5)[0],
                       np.zeros((16, 24), np.int32), np.full((16, 24), 7000, np.int32),
                       rng.integers(-(1 << 31), 1 << 31, (16, 24), dtype=np.int64).astype(np.int32)])
    planar = (3 * (np.arange(24)[None, :] - 12) + 480 * (np.arange(16)[:, None] - 8) + 200).astype(np.int32)[None]
    return {
        "scenes": (scenes, SMALL, base),
        "no refit": (scenes, SMALL, dataclasses.replace(base, refits=0)),
        "four refits, step 2": (scenes, dataclasses.replace(SMALL, step=2), dataclasses.replace(base, refits=4, min_inliers=5)),
        "step 4, a region": (scenes, dataclasses.replace(SMALL, step=4), dataclasses.replace(base, roi_x=1, roi_y=3, roi_w=22, roi_h=13, min_inliers=3)),
        "one row": (scenes, SMALL, dataclasses.replace(base, roi_x=0, roi_y=12, roi_w=24, roi_h=1)),
        "three samples": (scenes, SMALL, dataclasses.replace(base, roi_x=5, roi_y=10, roi_w=3, roi_h=1)),
        "a prior that is not level": (scenes, SMALL, dataclasses.replace(base, base_from_cam=obstacles.mount(0.3, 0.1, (0.2, -0.1, 0.6)))),
        "many inliers asked": (scenes, SMALL, dataclasses.replace(base, min_inliers=190)),
        "planar": (planar, SMALL, dataclasses.replace(base, tol_px=0.0, refits=1)),
        "tolerance 0": (scenes, SMALL, dataclasses.replace(base, tol_px=0.0)),
    }


SMALL_CASES = _small_cases()


@pytest.mark.parametrize("case", list(SMALL_CASES))
def test_twin_equals_the_plain_loop(case):
    raw, cam, p = SMALL_CASES[case]
    rec, lab = ground.reference(raw, cam, p)
    rec2, lab2 = ground.reference_loops(raw, cam, p)
    assert rec.tobytes() == rec2.tobytes(), (rec, rec2)
    assert np.array_equal(lab, lab2)
    if case == "scenes":      # the inputs do what they were built for
        assert [int(f) & ground.FOUND for f in rec["flags"][:3]] == [1, 1, 1] and not (rec["flags"][3:] & ground.FOUND).any()
        assert rec["flags"][3] == ground.NO_HYPOTHESIS and rec["usable"][3] == 0 and rec["winner"][3] == -1
        assert rec["flags"][4] == ground.NO_HYPOTHESIS and rec["usable"][4] == 24 * 8      # a wall: every hypothesis dies in the gate
        assert set(np.unique(lab[0])) >= {0, 1, 2} and np.all(lab[3] == 0) and np.all(lab[4] == 4)
    if case in ("one row", "three samples"):
        assert np.all(rec["flags"] == ground.NO_HYPOTHESIS)      # collinear samples span no plane
    if case == "many inliers asked":
        assert np.all(rec["flags"][:3] & ground.FEW_INLIERS) and np.all(rec["base_from_cam"] == f32(obstacles.LEVEL_MOUNT))
    if case == "planar":      # every live hypothesis counts every usable sample: the lowest live index wins
        r = rec[0]
        assert r["flags"] == ground.FOUND and r["inliers"] == r["usable"] and tuple(r["plane_q16"]) == (3 * 65536, 480 * 65536, 2120 * 65536)


def test_int64_arithmetic_holds_at_the_declared_limits():
    """Coordinates up to 8191 along either axis, disparities up to 2^24 and the largest tolerance: the plain loop works in Python
    integers (and asserts that its moments fit), the twin in int64 as the device does; they agree, so nothing wrapped."""
    rng = np.random.default_rng(2)
    p = GroundParams(hypotheses=24, refits=2, tol_px=8000.0, min_inliers=0, min_area=1, max_tilt_rad=1.5, height_min_m=1e-6, height_max_m=1e6,
                     roi_x=0, roi_y=0)
    assert ground.tol_raw(p) > 1 << 23
    for w, h in ((8192, 3), (3, 8192)):
        v, u = np.mgrid[0:h, 0:w]
        raw = (2000 * u + 100000 * v if w > h else 100000 * u + 2000 * v) + rng.integers(-4096, 4097, (h, w)) + 5000      # steep, but inside the gate
        raw[rng.random((h, w)) < 0.1] = 1 << 24
        raw[rng.random((h, w)) < 0.01] = (1 << 24) + 1
        raw = np.minimum(raw, (1 << 24) + 1).astype(np.int32)
        cam = Camera(fx=4000.0, fy=4000.0, cx=0.0, cy=0.0, baseline_mm=120.0)
        q = dataclasses.replace(p, roi_w=w, roi_h=h)
        g = ground.gate(cam, q, w, h)
        assert g[0] == -ground.SLOPE_LIM and g[3] == ground.SLOPE_LIM                  # the widest gate there is
        rec, _ = ground.reference(raw, cam, q, labels=False)
        rec2, _ = ground.reference_loops(raw, cam, q, labels=False)
        assert rec.tobytes() == rec2.tobytes() and rec["survivors"] > 0 and rec["inliers"] > 20000, (rec, rec2)


def _struct_fields(src, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            fields.append((m.group(1), ctype, int(m.group(2) or 1)))
    return fields


def test_header_structs_ctypes_mirrors_and_abi_version_agree():
    src = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()
    assert re.search(r"#define SN_ABI_VERSION (\d+)", src).group(1) == "4" and api.ABI_VERSION == 4
    ctypes_of = {"float": C.c_float, "int": C.c_int, "uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64}
    for name, mirror, size in (("sn_ground_params", api.SnGroundParams, 100), ("sn_ground", api.SnGround, 112)):
        fields = _struct_fields(src, name)
        assert [f for f, _, _ in fields] == [f for f, _ in mirror._fields_], name
        for (fname, ctype, count), (_, mtype) in zip(fields, mirror._fields_):
            assert mtype == (ctypes_of[ctype] * count if count > 1 else ctypes_of[ctype]), (name, fname)
        assert C.sizeof(mirror) == size
    # the numpy record is the struct, field for field, and the mount sits where the obstacle stage is told to look
    assert ground.RECORD.itemsize == C.sizeof(api.SnGround) == 4 * ground.RECORD_FLOATS
    for fname, _ in api.SnGround._fields_:
        assert ground.RECORD.fields[fname][1] == getattr(api.SnGround, fname).offset, fname
    assert api.SnGround.base_from_cam.offset == 4 * ground.MOUNT_OFFSET_FLOATS
    # the dataclass carries every field of the parameter struct (and the node's log_delta)
    assert [f for f, _ in api.SnGroundParams._fields_] + ["log_delta"] == [f.name for f in dataclasses.fields(GroundParams)]
    for k, v in (("FOUND", 1), ("NO_HYPOTHESIS", 2), ("FEW_INLIERS", 4), ("GATED", 8), ("SINGULAR", 16)):
        assert re.search(r"SN_GROUND_%s = (\d+)" % k, src).group(1) == str(v) == str(getattr(ground, k))
    for k, v in (("NONE", 0), ("GROUND", 1), ("ABOVE", 2), ("BELOW", 3), ("NO_PLANE", 4)):
        assert re.search(r"SN_GROUND_LABEL_%s = (\d+)" % k, src).group(1) == str(v) == str(getattr(ground, "LABEL_" + k))


def test_parameter_file_round_trip_and_errors(tmp_path):
    p = GroundParams(base_from_cam=obstacles.mount(0.1, 0.2, (0.3, 0.0, 0.45)), roi_x=4, roi_y=30, roi_w=80, roi_h=30, hypotheses=77, seed=4000000000,
                     min_area=9, min_inliers=123, refits=3, tol_px=0.07, max_tilt_rad=0.3, height_min_m=0.25, height_max_m=1.75, log_delta=0.005)
    path = str(tmp_path / "ground.txt")
    ground.save_params(path, p)
    assert ground.load_params(path) == p
    open(path, "w").write("hypotheses 12\n# a comment\n\ntol_px 0.5 # trailing\n")
    assert ground.load_params(path) == GroundParams(hypotheses=12, tol_px=0.5)
    for text in ("hypothesis 12\n", "hypotheses 12\nhypotheses 13\n", "base_from_cam 1 2 3\n", "tol_px x\n", "refits 1 2\n"):
        open(path, "w").write(text)
        with pytest.raises(ValueError):
            ground.load_params(path)


def test_gate_of_the_library_and_the_twin_and_what_it_holds():
    """The level prior's gate holds the level floor at every height of its range and no fronto-parallel wall; the library's gate
    is the twin's to within one (two implementations of a double cos and sin)."""
    p = GroundParams(max_tilt_rad=0.3, height_min_m=0.3, height_max_m=1.5)
    for cam, w, h in ((CAM, 96, 64), (dataclasses.replace(CAM, step=2), 96, 64), (Camera(fx=700.0, fy=690.0, cx=620.5, cy=180.25, baseline_mm=120.0), 1242, 375)):
        for prm in (p, dataclasses.replace(p, base_from_cam=obstacles.mount(0.2, 0.1, (0.0, 0.0, 0.7))), dataclasses.replace(p, roi_x=3, roi_y=40, roi_w=50, roi_h=11)):
            lib, twin = api.ground_gate(cam, prm, w, h), ground.gate(cam, prm, w, h)
            assert lib.dtype == np.int64 and np.all(np.abs(lib - twin) <= 1), (lib, twin)
            assert np.all(lib[0::2] <= lib[1::2])
    g = api.ground_gate(CAM, p, 96, 64)
    c, r, s = CAM, ground.roi(p, 96, 64, 1), float(ground.wire_scale())
    for hgt in (0.301, 0.5, 1.499):
        b = 0.12 / (hgt * s)                                                    # raw per row: the level floor is raw = b * (v - cy)
        q = (0.0, b * 65536, b * (r.v0 - c.cy) * 65536)
        assert all(g[2 * e] <= q[e] <= g[2 * e + 1] for e in range(3)), (hgt, q, g)
    assert not g[2] <= 0 <= g[3]                                                # a wall has b = 0
    assert not g[2] <= 0.12 / (0.25 * s) * 65536 <= g[3]                        # a floor nearer than height_min_m
    for bad in (dataclasses.replace(p, roi_x=90, roi_w=10, roi_y=0, roi_h=10), dataclasses.replace(p, hypotheses=0), dataclasses.replace(p, height_min_m=0.0),
                dataclasses.replace(p, max_tilt_rad=1.6), dataclasses.replace(p, tol_px=-1.0), dataclasses.replace(p, refits=5)):
        with pytest.raises(api.StereoNetError):
            api.ground_gate(CAM, bad, 96, 64)
        with pytest.raises(ValueError):
            ground.gate(CAM, bad, 96, 64)


def test_a_level_camera_half_a_metre_up_gives_back_the_level_mount():
    raw, _ = ground.scene(96, 64, CAM, 0.5)
    rec, lab = ground.reference(raw, CAM, GroundParams(hypotheses=32, tol_px=0.02, min_inliers=1000, min_area=16))
    assert rec["flags"] == ground.FOUND and rec["inliers"] == rec["usable"] == 96 * 31      # the row of the horizon holds nothing
    want = np.array(obstacles.LEVEL_MOUNT, np.float64)
    want[11] = 0.5
    assert np.abs(rec["base_from_cam"] - want).max() < 1e-5, rec["base_from_cam"]
    assert np.abs(rec["plane_cam"] - np.array([0, 1, 0, 0.5])).max() < 1e-5
    assert np.all(lab[33:] == ground.LABEL_GROUND) and np.all(lab[:33] == ground.LABEL_NONE)
    pitch, roll = ground.angles(rec["base_from_cam"])
    assert abs(pitch) < 1e-5 and abs(roll) < 1e-5
    # the mount keeps the prior's heading and horizontal offset
    prior = obstacles.mount(0.4, 0.0, (0.3, -0.2, 0.9))
    rec2, _ = ground.reference(raw, CAM, GroundParams(base_from_cam=prior, hypotheses=32, tol_px=0.02, min_inliers=1000, min_area=16), labels=False)
    assert rec2["flags"] == ground.FOUND
    assert np.abs(rec2["base_from_cam"] - np.array(obstacles.mount(0.4, 0.0, (0.3, -0.2, 0.5)))).max() < 1e-5


DRAWS = 45


def _draw(seed):
    rng = np.random.default_rng(seed)
    hgt, pitch, roll = rng.uniform(0.3, 1.2), rng.uniform(-0.05, 0.35), rng.uniform(-0.15, 0.15)
    raw, floor = ground.scene(96, 64, CAM, hgt, pitch, roll, wall_z_m=rng.uniform(3.0, 8.0), boxes=2, hole_frac=0.10, outlier_frac=0.15, seed=seed)
    return raw, floor, hgt, pitch, roll


def test_geometric_truth_on_seeded_scenes():
    """45 draws: height 0.3 .. 1.2 m, pitch -0.05 .. 0.35 rad, roll +-0.15 rad, a wall, two boxes, 15 % outliers, 10 % holes,
    tol_px = 0.02, K = 128, two refits.  Every draw is found, the height to 0.5 % and the normal to 0.1 degree of the constructed
    values (the map's quantisation and the fit leave an order of magnitude: the bounds catch a wrong sign, axis or unit).
    Measured: worst height error 3.9e-4, worst angle 0.014 degree."""
    p = GroundParams(hypotheses=128, refits=2, tol_px=0.02, min_inliers=50, min_area=16)
    worst_h = worst_a = 0.0
    for seed in range(DRAWS):
        raw, floor, hgt, pitch, roll = _draw(seed)
        assert floor[32:].mean() >= 0.25, (seed, "the floor holds less than a quarter of the region")
        rec, lab = ground.reference(raw, CAM, p)
        assert rec["flags"] & ground.FOUND, (seed, rec)
        n = ground.plane_normal(pitch, roll)
        err_h = abs(float(rec["plane_cam"][3]) / hgt - 1.0)
        err_a = math.degrees(math.acos(min(1.0, float(np.dot(rec["plane_cam"][:3].astype(np.float64), n)))))
        worst_h, worst_a = max(worst_h, err_h), max(worst_a, err_a)
        assert err_h <= 5e-3 and err_a <= 0.1, (seed, err_h, err_a)
        got_pitch, got_roll = ground.angles(rec["base_from_cam"])
        assert abs(got_pitch - pitch) < 2e-3 and abs(got_roll - roll) < 2e-3 and abs(float(rec["base_from_cam"][11]) / hgt - 1.0) <= 5e-3
        assert (lab[floor] == ground.LABEL_GROUND).mean() > 0.95, seed           # what the scene calls floor, the labels call ground
    print(f"worst height error {worst_h:.2e}, worst angle {worst_a:.4f} degree over {DRAWS} draws")


def test_without_the_gate_the_wall_can_win():
    """what the gate is for: with the gate opened to everything, some scene's largest plane is its wall"""
    p = GroundParams(hypotheses=128, refits=0, tol_px=0.02, min_inliers=50, min_area=16)
    open_gate = np.array([-ground.SLOPE_LIM, ground.SLOPE_LIM, -ground.SLOPE_LIM, ground.SLOPE_LIM, -ground.OFFSET_LIM, ground.OFFSET_LIM])
    walls = 0
    for seed in range(12):
        raw, floor = ground.scene(96, 64, CAM, 0.8, 0.1, 0.0, wall_z_m=2.0, outlier_frac=0.05, seed=seed)
        assert 0.25 < floor[32:].mean() < 0.4                                   # the wall holds more of the region than the floor
        gated, _ = ground.reference(raw, CAM, p, labels=False)
        free, _ = ground.reference(raw, CAM, p, gate_q16=open_gate, labels=False)
        assert gated["flags"] & ground.FOUND and abs(float(gated["plane_cam"][3]) - 0.8) < 4e-3
        walls += abs(int(free["plane_q16"][1])) < 65536                          # a plane whose disparity does not change with the row
    assert walls >= 6


def test_a_floor_of_a_few_per_cent_is_refused_with_the_prior_mount():
    prior = obstacles.mount(0.0, 0.05, (0.1, 0.0, 0.55))
    p = GroundParams(base_from_cam=prior, hypotheses=1024, refits=2, tol_px=0.02, min_inliers=300, min_area=16)
    for seed in range(8):
        rng = np.random.default_rng(100 + seed)
        raw, floor = ground.scene(96, 64, CAM, 0.5, 0.05, seed=seed)
        keep = rng.random((64, 96)) < 0.05
        raw = np.where(keep, raw, rng.integers(200, 20000, (64, 96))).astype(np.int32)
        assert 0.02 < (keep & floor)[32:].mean() < 0.08
        rec, lab = ground.reference(raw, CAM, p)
        assert int(rec["flags"]) & ~ground.SINGULAR == ground.FEW_INLIERS and rec["inliers"] < 300 and rec["survivors"] > 0, (seed, rec)
        assert np.array_equal(rec["base_from_cam"], f32(prior)) and np.array_equal(rec["plane_cam"], f32([-prior[8], -prior[9], -prior[10], prior[11]]))
        assert np.all(lab[raw > 0] == ground.LABEL_NO_PLANE) and np.all(lab[raw <= 0] == ground.LABEL_NONE)
