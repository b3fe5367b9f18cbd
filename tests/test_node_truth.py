"""The node's published messages against float64 scene geometry.  tests/test_chain_truth.py holds the chain to the analytic
world of tests/golden/scene_truth.py through api.*, with the glue between the stages (the goal's cell less the window's origin,
the rollout's origin, the yaws, the mounts) written on the test's side.  stereonet_node.cpp writes that glue a second time, and a
robot consumes its messages and nothing else.  Here the messages themselves are decoded by tests/golden/node_messages.py, which
knows the ROS conventions and nothing of the product, and are held to the same truth with the same bounds: the checks are
test_chain_truth's, taking cell centres in metres and values instead of the api's arrays.

This file proves the test's own logic where there is no GPU: decoder, checks and teeth run on
node_messages.messages_from_chain(twin_chain(name)), what a correct node publishes for the twins' chain.
tests/test_gpu_node_truth.py runs the same checks on what csrc/compat/test/scene_harness.cpp recorded of the real node.

Tolerances.  test_chain_truth's dZ, E, D, the grid, map, cost and arc bounds, unchanged.  New here, none from an output:
  origin   info.origin of the costmap is the truth's corner of cell (0, 0) to 2/256 cell per axis: the pose is quantised to
           1/256 cell, a product of an integer and the fp32 cell is exact to 2^-53, the rest is slack below one quantum; held
           on the coordinates of a pose that keep 2/256 cell from a cell's border, both of the last frame among them;
  ends     a path's pose is a cell's centre and the robot (the goal) lies in that cell: half the cell's diagonal, + 1e-9 m for the
           float64 sums;
  lattice  |v - lattice| <= 2^-22 max(|v_min|, |v_max|): the two parameters are fp32 (2^-24 relative each), the lattice is
           made of them in double;
  heading  a yaw equals the arc's heading to 2 units of 1/65536 turn, check_rollout's bound on the heading word (the quaternion
           is sin and cos of traj[..2] / 65536 * pi in double: 1e-15 more);
  unit     |z^2 + w^2 - 1| <= 2^-50: sin^2 + cos^2 of one double, each rounded;
  scan     angle_max against angle_min + (beams - 1/2) increment of the file in double, to 2^-21 (|angle_min| + beams
           |increment|): two fp32 parameters and three fp32 operations on values no larger than that sum, 2^-24 each, rounded
           up to a power of two; range_min and range_max are the file's to one fp32 rounding, 2^-24 relative;
  cloud    a point is its pixel's hit in the camera frame to dz = Z / (2 r - 1), the exact form of dZ for the ray's own depth (r =
           the unrounded map value; raw is within 1/2 of it, so Z' = Z r / raw <= Z r / (r - 1/2); depth_half_step is its first
           order), scaled along the ray: |u - cx| / fx dz in X, |v - cy| / fy dz in Y; + 2^-21 of the coordinate for the five
           fp32 operations of the documented formula.
"""
import dataclasses
import functools
import math
import os
import subprocess
import types

import numpy as np
import pytest

import node_messages as nm
import scene_truth as st
import test_chain_truth as ct
from hobot_stereonet_amd.spec import OUT_SCALE

TAG = "node_truth"
COMPAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hobot_stereonet_amd", "csrc", "compat")
CLOUD_Z = (0.25, 8.0)                       # STEREONET_POINTCLOUD_Z: the nearest ground the camera sees is 1 m away, the walls end within 8 m
CAM = dataclasses.replace(st.CAM, z_min_m=CLOUD_Z[0], z_max_m=CLOUD_Z[1])
# each misreading of the messages and the check that must catch it
CAUGHT_BY = {"the grid read column-major": "grid", "the origin taken as the window's centre": "costmap", "the origin's y negated": "grid",
             "beam order reversed": "scan", "angle_min taken as the sector's edge": "scan", "angular.z negated": "command",
             "the quaternion's z negated": "command", "cloud X and Y swapped": "cloud"}
assert set(CAUGHT_BY) == set(nm.MISREADINGS)


def node_params(scene):
    """the parameter blocks a node of this scene is started with"""
    rp = dataclasses.replace(ct.RP, footprint=tuple(map(tuple, ct.FOOTPRINT.astype(np.float64).tolist())))
    return types.SimpleNamespace(op=ct.OP, cp=ct.costmap_params(scene), ip=ct.IP, nav=ct.NAV, rp=rp, gp=ct.GP, cam=CAM, out_scale=OUT_SCALE)


def _stamp(k):
    return (nm.STAMP_SEC, nm.STAMP_NANOSEC + k)


def _frames(name, M, kind):
    scene = st.SCENES[name]
    assert len(M[kind]) == len(scene.poses), (kind, len(M[kind]), len(scene.poses))
    return scene, list(zip(scene.poses, M[kind]))


# ---- the checks: each takes a scene's name, its messages and a decoder, prints its node_truth line and asserts -------------------------
def check_grid(name, M, dec):
    """/stereonet_obstacle_grid, frame by frame: grid_bounds' two directions on the decoded cell centres, taken to the world by the
    true pose; the obstacle frame's id and the injected stamp"""
    scene, frames = _frames(name, M, "grid")
    occupied = []
    for k, (pose, msg) in enumerate(frames):
        assert msg["frame_id"] == ct.OP.frame and msg["stamp"] == _stamp(k) and msg["load"] == _stamp(k), (k, msg["frame_id"], msg["stamp"])
        centres, values = dec.grid(msg)
        assert values.shape == (ct.OP.gh, ct.OP.gw) and set(np.unique(values)) <= {-1, 0, 100}
        occupied.append(nm.from_frame(pose, centres[values == 100]))
    ct.grid_bounds(name, occupied, lambda k, xy: dec.grid_at(M["grid"][k], xy) == 100, tag=TAG)


def check_scan(name, M, dec):
    """/stereonet_scan: scan_bounds with beam i's sector from angle_min, angle_increment and i alone; the other scalars against
    the parameter file"""
    scene, frames = _frames(name, M, "scan")
    op = ct.OP
    angles = dec.scan(M["scan"][0])[0]
    inc = float(M["scan"][0]["angle_increment"])
    ranges = []
    for k, (pose, msg) in enumerate(frames):
        assert msg["frame_id"] == op.frame and msg["stamp"] == _stamp(k), (k, msg["frame_id"], msg["stamp"])
        a, r = dec.scan(msg)
        assert len(r) == op.beams and np.array_equal(a, angles) and msg["intensities"] == 0
        want = op.angle_min_rad + (op.beams - 0.5) * op.angle_increment_rad
        assert abs(msg["angle_max"] - want) <= 2.0 ** -21 * (abs(op.angle_min_rad) + op.beams * abs(op.angle_increment_rad)), (msg["angle_max"], want)
        assert abs(msg["range_min"] - op.range_min_m) <= 2.0 ** -24 * abs(op.range_min_m) and abs(msg["range_max"] - op.range_max_m) <= 2.0 ** -24 * abs(op.range_max_m)
        assert msg["time_increment"] == 0.0 and msg["scan_time"] == 0.0
        # a return lies between range_min and range_max; no return is not a finite number
        assert np.all((r[np.isfinite(r)] >= msg["range_min"]) & (r[np.isfinite(r)] <= msg["range_max"]))
        ranges.append(r)
    ct.scan_bounds(name, ranges, lambda b: (angles[b] - 0.5 * inc, angles[b] + 0.5 * inc), tag=TAG)


def _state(values):
    return np.where(values == -1, ct.UNKNOWN, np.where(values >= ct.LETHAL_MIN, ct.OCCUPIED, ct.FREE)).astype(np.int8)


def check_costmap(name, M, dec):
    """/stereonet_costmap: info.origin of every frame is the truth's corner; costmap_bounds (and scroll_bounds on the clip that
    re-centres) on the last frame's int8 values: unknown is -1, occupied a value >= LETHAL_MIN, free the rest"""
    T = ct.truth(name)
    scene, frames = _frames(name, M, "costmap")
    mw, mh = scene.window
    for k, (pose, msg) in enumerate(frames):
        assert msg["frame_id"] == ct.CP.frame and msg["stamp"] == _stamp(k) and msg["load"] == _stamp(k), (k, msg["frame_id"], msg["stamp"])
        assert (msg["width"], msg["height"]) == (mw, mh) and msg["resolution"] == ct.CELL
        o = msg["origin"]
        assert tuple(o[2:]) == (0.0, 0.0, 0.0, 0.0, 1.0), ("the origin's pose is not the identity at z = 0", o)
    # a coordinate within a quantum of a cell's border may be rounded into either cell: there the origin is not held (the last
    # pose of every scene lies on a cell's centre)
    frac = np.array([[(p / ct.CELL) % 1.0 for p in pose[:2]] for pose in scene.poses])
    held = (frac > 2.0 / 256.0) & (frac < 1.0 - 2.0 / 256.0)      # per frame and axis
    assert held[-1].all(), held
    corner = np.array([dec.grid(msg)[0][0, 0] for msg in M["costmap"]]) - 0.5 * ct.CELL      # of cell (0, 0), as the decoder places it
    off = float(np.abs(corner - np.asarray(T["origins"], np.float64) * ct.CELL)[held].max() / ct.CELL * 256.0)
    print(f"{TAG} {name} | origin | the corner of cell (0, 0) off the truth's by {off:.4f} <= 2 units of 1/256 cell over {int(held.sum())} of {held.size} coordinates")
    assert off <= 2.0, off
    centres, values = dec.grid(M["costmap"][-1])
    ct.costmap_bounds(name, centres, _state(values), tag=TAG)
    if scene.window != (100, 100):
        truth_centres = st.cell_centres(T["origins"][-1], ct.CELL, mw, mh)
        ct.scroll_bounds(name, dec.grid_at(M["costmap"][-1], truth_centres) != -1, tag=TAG)


def check_inflation(name, M, dec):
    """/stereonet_inflated_grid: the header and info of its source; inflation_bounds on the published values, which the
    documented translation maps 253 -> 99, 254 -> 100 and everything lower, or unknown, to something else"""
    src, msg = M["costmap"][-1], M["inflated"][-1]
    for key in ("frame_id", "stamp", "load", "resolution", "width", "height", "origin"):
        assert msg[key] == src[key], (key, msg[key], src[key])
    centres, values = dec.grid(msg)
    assert values.min() >= -1 and values.max() <= 100
    ct.inflation_bounds(name, centres, (values != 99) & (values != 100), tag=TAG)


def _path_header_ok(msg, src):
    return (msg["frame_id"] == src["frame_id"] and msg["stamp"] == src["stamp"] and all(f == msg["frame_id"] for f in msg["pose_frame_ids"]) and
            all(s == msg["stamp"] for s in msg["pose_stamps"]))


def check_plan(name, M, dec):
    """/stereonet_plan: path_bounds (the opening, the geodesic, the witness, the clearance) on the published positions; the ends
    within half a cell's diagonal of the robot and of the goal; the header of the source on the path and on every pose"""
    scene = st.SCENES[name]
    msg = M["plan"][-1]
    assert _path_header_ok(msg, M["costmap"][-1]), "a pose or the path without the source's header"
    xy, yaw, q = dec.path(msg)
    assert len(xy) > 1, "the plan has one pose or none"
    assert np.all(np.asarray(msg["positions"])[:, 2] == 0.0) and np.all(q == (0.0, 0.0, 0.0, 1.0))
    ends = (float(np.hypot(*(xy[0] - scene.poses[-1][:2]))), float(np.hypot(*(xy[-1] - np.asarray(scene.goal)))))
    bound = ct.SQ2 / 2 * ct.CELL + 1e-9
    print(f"{TAG} {name} | ends | first pose {ends[0]:.4f} m from the robot, last {ends[1]:.4f} m from the goal, both <= {bound:.4f} m")
    assert max(ends) <= bound, ends
    ct.path_bounds(name, xy, tag=TAG)


def check_command(name, M, dec, rp=None):
    """/stereonet_cmd_vel and /stereonet_local_plan: the Twist is a lattice value with nothing beside linear.x and angular.z and is
    no stop; the closed-form arc of it from the true pose stays within arc_bounds of the local plan's positions and yaws; every
    quaternion is a unit yaw quaternion; the command turns to the side the scene says"""
    scene = st.SCENES[name]
    rp = rp or ct.RP
    v, w, rest = dec.twist(M["cmd"][-1])
    assert rest == (0.0, 0.0, 0.0, 0.0), rest
    lv, lw = nm.lattice(rp)
    dv, dw = float(np.abs(lv - v).min()), float(np.abs(lw - w).min())
    bv, bw = 2.0 ** -22 * max(abs(rp.v_min), abs(rp.v_max)), 2.0 ** -22 * max(abs(rp.w_min), abs(rp.w_max))
    print(f"{TAG} {name} | command | v {v:.3f} m/s off the lattice by {dv:.2e} <= {bv:.2e}, w {w:+.2f} rad/s by {dw:.2e} <= {bw:.2e}")
    assert dv <= bv and dw <= bw, (v, w)
    assert (v, w) != (0.0, 0.0), "the command is a stop"
    msg = M["local_plan"][-1]
    assert _path_header_ok(msg, M["costmap"][-1]), "a pose or the local plan without the source's header"
    xy, yaw, q = dec.path(msg)
    assert len(xy) > 1, "the local plan has one pose or none"
    assert np.all(np.asarray(msg["positions"])[:, 2] == 0.0) and np.all(q[:, :2] == 0.0), "not a rotation about z at z = 0"
    assert np.abs(q[:, 2] ** 2 + q[:, 3] ** 2 - 1.0).max() <= 2.0 ** -50, "not a unit quaternion"
    ct.arc_bounds(name, v, w, xy, yaw / (2 * math.pi), tag=TAG)
    if scene.left:
        assert v > 0 and w * scene.left > 0, ("the command does not turn towards the way round", v, w)


def camera_frame(scene, pose, pts):
    """world points (..., 3) in the optical frame of the scene's camera at a pose: X right, Y down, Z forward"""
    b = st.to_base(pose, pts[..., :2])
    bx, left, bz = b[..., 0], b[..., 1], pts[..., 2] - scene.cam_height
    cp, sp = math.cos(scene.pitch), math.sin(scene.pitch)
    fwd, up = cp * bx - sp * bz, sp * bx + cp * bz      # the camera is pitched down: its forward axis tips towards -z
    return np.stack([-left, -up, fwd], -1)


def check_cloud(name, M, dec):
    """/stereonet_pointcloud2 (organised, the scene's camera): every finite point is its pixel's hit in the camera frame; a pixel
    without a hit is no finite point; at least 90 % of the wall and ground pixels inside the Z range are finite points"""
    scene, frames = _frames(name, M, "cloud")
    cam = CAM
    u, v = np.meshgrid(np.arange(st.W, dtype=np.float64), np.arange(st.H, dtype=np.float64))
    sx, sy = np.abs(u - cam.cx) / cam.fx, np.abs(v - cam.cy) / cam.fy
    worst, share_min = 0.0, 1.0
    for k, (pose, msg) in enumerate(frames):
        assert msg["frame_id"] == str(nm.FRAME_INDEX + k) and msg["stamp"] == _stamp(k), (k, msg["frame_id"], msg["stamp"])
        assert (msg["height"], msg["width"]) == (st.H, st.W) and not msg["is_dense"]
        got = dec.cloud(msg)
        finite = np.isfinite(got).all(-1)
        assert np.array_equal(finite, np.isfinite(got).any(-1)), "a point that is finite in part"
        pts, label, depth = st.hit_points(scene, pose)
        assert not (finite & (label == st.NONE)).any(), "a finite point where no ray hits anything"
        want = camera_frame(scene, pose, pts)
        with np.errstate(invalid="ignore", divide="ignore"):
            z = np.where(label != st.NONE, depth, np.nan)
            assert np.nanmax(np.abs(want[..., 2] - z)) < 1e-9 and np.nanmax(np.abs(want[..., 0] - (u - cam.cx) / cam.fx * z)) < 1e-9      # the frames agree
            r = cam.fx * cam.baseline_mm / (z * 192000.0) / OUT_SCALE
            dz = z / (2.0 * r - 1.0)
            bound = np.stack([sx * dz, sy * dz, dz], -1) + 2.0 ** -21 * np.abs(want)
            over = np.abs(got - want) / bound
        worst = max(worst, float(over[finite].max()))
        inside = (label != st.NONE) & (z - dz >= CLOUD_Z[0]) & (z + dz <= CLOUD_Z[1])
        outside = (label != st.NONE) & ((z + dz < CLOUD_Z[0]) | (z - dz > CLOUD_Z[1]))
        assert not (finite & outside).any(), "a finite point outside the Z range"
        share_min = min(share_min, float((finite & inside).sum() / inside.sum()))
    print(f"{TAG} {name} | cloud | the finite points use {worst:.3f} <= 1 of their bounds | finite among the hits inside the Z range {share_min:.3f} >= 0.9")
    assert worst <= 1.0 and share_min >= 0.9, (worst, share_min)


CHECKS = {"grid": check_grid, "scan": check_scan, "costmap": check_costmap, "inflation": check_inflation, "plan": check_plan, "command": check_command,
          "cloud": check_cloud}


def failures(name, M, dec, checks=CHECKS):
    """the names of the checks that fail, with why"""
    out = {}
    for label, fn in checks.items():
        try:
            fn(name, M, dec)
        except AssertionError as e:
            out[label] = str(e)[:200]
    return out


def occupied_cells(M, dec):
    """the world cells that the last costmap message gives as occupied"""
    centres, values = dec.grid(M["costmap"][-1])
    return np.floor(centres[values >= ct.LETHAL_MIN] / ct.CELL).astype(np.int64)


def check_mirror(a, b, Ma, Mb, dec):
    """check_mirror's statement on the decoded messages of a scene and of its mirror image"""
    ct.mirror_bounds(a, occupied_cells(Ma, dec), occupied_cells(Mb, dec), dec.twist(Ma["cmd"][-1])[:2], dec.twist(Mb["cmd"][-1])[:2], tag=TAG)


# ---- the far pose: where the plan's glue and the costmap's could part ---------------------------------------------------------------------
FAR_CELL = (30000, -30000)                                    # 3 km from the origin
FAR_POSE = (FAR_CELL[0] * ct.CELL, FAR_CELL[1] * ct.CELL, 0.0)      # on the cell's lower edge in x and y, as exactly as a double says it


def check_far_pose(M, dec, window):
    """One frame at FAR_POSE.  The pose lies on the border between two cells; by the costmap's contract (tx = llrint(x * 256 /
    cell), the cell is tx >> 8) it is in FAR_CELL, which is also floor(x / cell) in exact arithmetic, and the window's element
    [mh / 2][mw / 2] is that cell.  The plan's first pose is the centre of the robot's cell: the same cell."""
    mw, mh = window
    centres, _ = dec.grid(M["costmap"][-1])
    corner = centres[0, 0] - 0.5 * ct.CELL
    want = (np.asarray(FAR_CELL) - (mw // 2, mh // 2)) * ct.CELL
    off = float(np.abs(corner - want).max() / ct.CELL * 256.0)
    xy = dec.path(M["plan"][-1])[0]
    first = xy[0] / ct.CELL - 0.5
    print(f"{TAG} far pose | origin | the corner of cell (0, 0) off the truth's by {off:.4f} <= 2 units of 1/256 cell | the plan starts in cell "
          f"({first[0]:.6f}, {first[1]:.6f}), the robot stands in {FAR_CELL}")
    assert off <= 2.0, off
    # a cell's index as a double of this size is exact to 2^-37: 1e-6 tells one cell from the next
    assert np.abs(first - FAR_CELL).max() <= 1e-6, (first, FAR_CELL)


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_messages(name):
    """what a correct node publishes for the twins' chain of a scene, computed once and shared"""
    scene = st.SCENES[name]
    return nm.messages_from_chain(ct.twin_chain(name), scene, node_params(scene))


def test_compat_builds_the_scene_harness():
    from hobot_stereonet_amd import build
    build.build()
    subprocess.check_call(["make", "-C", COMPAT, "-s", "build/scene_harness"])
    assert os.path.exists(os.path.join(COMPAT, "build", "scene_harness"))
    assert subprocess.run([os.path.join(COMPAT, "build", "scene_harness")], capture_output=True).returncode == 2      # the usage line, no node


@pytest.mark.parametrize("name", list(st.SCENES))
def test_reference_messages_against_the_truth(name):
    """decoder and checks on the reference publisher: every check passes on what a correct node says of the twins' chain"""
    bad = failures(name, reference_messages(name), nm.Decoder())
    assert not bad, bad


@pytest.mark.parametrize("name", ["free end", "gap and box", "corridor", "free end pitched"])
def test_the_mirrored_world_in_messages(name):
    check_mirror(name, name + " mirrored", reference_messages(name), reference_messages(name + " mirrored"), nm.Decoder())


@pytest.mark.parametrize("misread", list(CAUGHT_BY))
def test_every_misreading_is_caught(misread):
    """the checks have teeth: each convention of the messages read wrongly fails the check that is there for it"""
    bad = failures("free end", reference_messages("free end"), nm.Decoder(misread))
    print(f"{TAG} free end | misreading | {misread}: caught by {sorted(bad)}")
    assert CAUGHT_BY[misread] in bad, (misread, bad)


def test_the_decoder_on_known_messages():
    """the decoder against messages written out by hand: a grid that is not square and stands turned in its frame, a scan, a
    quarter turn, a cloud with its fields in an order of its own"""
    dec = nm.Decoder()
    half = math.sqrt(0.5)
    grid = dict(resolution=0.5, width=3, height=2, origin=(1.0, 2.0, 0.0, 0.0, 0.0, half, half), data=np.arange(6, dtype=np.int8))      # turned by +90 degrees
    centres, values = dec.grid(grid)
    assert values.tolist() == [[0, 1, 2], [3, 4, 5]]
    assert np.allclose(centres[0, 0], (0.75, 2.25)) and np.allclose(centres[0, 2], (0.75, 3.25)) and np.allclose(centres[1, 0], (0.25, 2.25))
    assert dec.grid_at(grid, np.array([(0.75, 3.25), (0.25, 2.25), (1.1, 2.1)])).tolist() == [2, 3, -1]
    a, r = dec.scan(dict(angle_min=-0.5, angle_increment=0.25, ranges=np.float32([1, 2, 3])))
    assert a.tolist() == [-0.5, -0.25, 0.0] and r.tolist() == [1.0, 2.0, 3.0]
    assert abs(nm.yaw_of((0.0, 0.0, half, half)) - math.pi / 2) < 1e-15 and abs(nm.yaw_of((0.0, 0.0, -half, half)) + math.pi / 2) < 1e-15
    assert np.allclose(nm.from_frame((1.0, 1.0, math.pi / 2), (1.0, 0.0)), (1.0, 2.0)) and np.allclose(nm.into_frame((1.0, 1.0, math.pi / 2), (1.0, 2.0)), (1.0, 0.0))
    pts = np.zeros((2, 1), np.dtype([("pad", "<u2"), ("z", "<f8"), ("y", "<f4"), ("x", "<f4"), ("tail", "<u2")]))
    pts["x"], pts["y"], pts["z"] = [[1.0], [4.0]], [[2.0], [5.0]], [[3.0], [6.0]]
    cloud = dict(height=2, width=1, point_step=20, row_step=20, is_bigendian=False, data=pts.tobytes(),
                 fields=[("z", 2, 8, 1), ("y", 10, 7, 1), ("x", 14, 7, 1)])
    assert dec.cloud(cloud).tolist() == [[[1.0, 2.0, 3.0]], [[4.0, 5.0, 6.0]]]


def test_the_far_pose_in_exact_arithmetic():
    """what check_far_pose rests on: FAR_POSE is on the border (x / cell is the integer to within the double's rounding) and the
    contract's tx >> 8 puts it in FAR_CELL; and the check passes on a correct node's messages"""
    from fractions import Fraction
    for x, c in zip(FAR_POSE[:2], FAR_CELL):
        assert abs(Fraction(x) / Fraction(ct.CELL) - c) < Fraction(1, 2 ** 30)
        assert round(x * (256.0 / ct.CELL)) >> 8 == c
    mw, mh = 100, 100
    ox, oy = FAR_CELL[0] - mw // 2, FAR_CELL[1] - mh // 2
    M = dict(costmap=[dict(resolution=ct.CELL, width=mw, height=mh, origin=(ox * ct.CELL, oy * ct.CELL, 0, 0, 0, 0, 1), data=np.zeros(mw * mh, np.int8))],
             plan=[dict(positions=np.array([[(FAR_CELL[0] + 0.5) * ct.CELL, (FAR_CELL[1] + 0.5) * ct.CELL, 0.0]]), orientations=np.array([[0.0, 0, 0, 1]]))])
    check_far_pose(M, nm.Decoder(), (mw, mh))
    M["plan"][0]["positions"][0, 0] -= ct.CELL      # the cell next to it
    with pytest.raises(AssertionError):
        check_far_pose(M, nm.Decoder(), (mw, mh))
