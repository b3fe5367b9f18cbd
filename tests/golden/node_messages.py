"""What the node's messages say, read by nothing but what ROS fixes, in float64 and plain numpy (tests/test_node_truth.py,
tests/test_gpu_node_truth.py).

A message here is a dict of the message's own fields (`load_recording` makes them of what scene_harness recorded,
`messages_from_chain` of what a chain computed).  The decoder turns them into metres and radians in the frame of the message's
header, with these conventions and no other:
  REP-103: x forward, y left, z up; a yaw is counter-clockwise seen from above.
  nav_msgs/OccupancyGrid: data is row-major from cell (0, 0), x along the width: data[j * width + i] is cell (i, j); info.origin
    is the pose of the outer corner of cell (0, 0), so the cell covers origin + R(yaw) ([i, i + 1) res, [j, j + 1) res).
  sensor_msgs/LaserScan: beam i looks along angle_min + i * angle_increment, so what it saw lies within half an increment of that.
  geometry_msgs/Quaternion (x, y, z, w): the rotation by 2 acos(w) about (x, y, z); its yaw is atan2(2 (w z + x y), 1 - 2 (y y + z z)).
  sensor_msgs/PointCloud2: point (row r, column c) starts at data[r * row_step + c * point_step]; a field lies at its `offset`
    from there in the type its `datatype` names, in the byte order is_bigendian names.  An optical frame is X right, Y down, Z forward.
Nothing here comes from a twin, from api.* or from the node's comments: of the package only parameter dataclasses are read,
and only by messages_from_chain.

`Decoder(misread)` reads the messages wrongly in one of MISREADINGS' ways: the tests show that each is caught.

messages_from_chain is the other half: what a correct node publishes for a chain's result, written from the documentation in
stereonet_node.h (which topics, which header, which frame) and include/stereonet_hip.h (what the arrays mean).
"""
from __future__ import annotations

import math
import re

import numpy as np

MISREADINGS = ("the grid read column-major", "the origin taken as the window's centre", "the origin's y negated", "beam order reversed",
               "angle_min taken as the sector's edge", "angular.z negated", "the quaternion's z negated", "cloud X and Y swapped")
STAMP_SEC, STAMP_NANOSEC, FRAME_INDEX = 7, 1000, 100      # frame k is stamped 7.(1000 + k) and named "100 + k", by scene_harness and here
_FIELD_TYPES = {1: "i1", 2: "u1", 3: "i2", 4: "u2", 5: "i4", 6: "u4", 7: "f4", 8: "f8"}      # sensor_msgs/PointField


def yaw_of(q) -> np.ndarray:
    """the yaw of quaternions (..., 4) = x, y, z, w"""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))


def from_frame(pose, xy) -> np.ndarray:
    """points (..., 2) of a frame that stands at pose = (x, y, yaw) of a parent frame -> in the parent frame"""
    p = np.asarray(xy, np.float64)
    c, s = math.cos(pose[2]), math.sin(pose[2])
    return np.stack([pose[0] + c * p[..., 0] - s * p[..., 1], pose[1] + s * p[..., 0] + c * p[..., 1]], -1)


def into_frame(pose, xy) -> np.ndarray:
    """the inverse of from_frame"""
    p = np.asarray(xy, np.float64) - (pose[0], pose[1])
    c, s = math.cos(pose[2]), math.sin(pose[2])
    return np.stack([c * p[..., 0] + s * p[..., 1], -s * p[..., 0] + c * p[..., 1]], -1)


class Decoder:
    def __init__(self, misread=None):
        assert misread is None or misread in MISREADINGS, misread
        self.misread = misread

    # ---- nav_msgs/OccupancyGrid
    def _grid_pose(self, msg):
        o = msg["origin"]
        res, w, h = float(msg["resolution"]), int(msg["width"]), int(msg["height"])
        pose = [float(o[0]), float(o[1]), float(yaw_of(o[3:7]))]
        if self.misread == "the origin's y negated":
            pose[1] = -pose[1]
        if self.misread == "the origin taken as the window's centre":
            pose[0], pose[1] = from_frame(pose, (-0.5 * w * res, -0.5 * h * res))
        return pose, res, w, h

    def _grid_values(self, msg, w, h):
        data = np.asarray(msg["data"], np.int8).astype(np.int64)
        assert data.size == w * h, (data.size, w, h)
        return data.reshape(w, h).T if self.misread == "the grid read column-major" else data.reshape(h, w)

    def grid(self, msg):
        """-> (centres float64 (height, width, 2), values int64 (height, width)): element [j][i] is cell (i, j), its centre in
        the header's frame"""
        pose, res, w, h = self._grid_pose(msg)
        i, j = np.meshgrid(np.arange(w), np.arange(h))
        return from_frame(pose, np.stack([(i + 0.5) * res, (j + 0.5) * res], -1)), self._grid_values(msg, w, h)

    def grid_at(self, msg, xy, outside=-1):
        """the value of the cell that holds each point xy (..., 2) of the header's frame; `outside` off the grid"""
        pose, res, w, h = self._grid_pose(msg)
        p = into_frame(pose, xy)
        i, j = np.floor(p[..., 0] / res).astype(np.int64), np.floor(p[..., 1] / res).astype(np.int64)
        inside = (i >= 0) & (i < w) & (j >= 0) & (j < h)
        return np.where(inside, self._grid_values(msg, w, h)[np.clip(j, 0, h - 1), np.clip(i, 0, w - 1)], outside)

    # ---- sensor_msgs/LaserScan
    def scan(self, msg):
        """-> (angles float64 (n,): where each beam looks, in the header's frame; ranges float64 (n,))"""
        r = np.asarray(msg["ranges"], np.float32).astype(np.float64)
        a = float(msg["angle_min"]) + np.arange(len(r)) * float(msg["angle_increment"])
        if self.misread == "angle_min taken as the sector's edge":
            a = a + 0.5 * float(msg["angle_increment"])
        if self.misread == "beam order reversed":
            r = r[::-1]
        return a, r

    # ---- nav_msgs/Path
    def path(self, msg):
        """-> (xy float64 (n, 2), yaw float64 (n,), quaternions float64 (n, 4) = x, y, z, w as read)"""
        pos = np.asarray(msg["positions"], np.float64).reshape(-1, 3)
        q = np.array(msg["orientations"], np.float64).reshape(-1, 4)
        if self.misread == "the quaternion's z negated":
            q[:, 2] = -q[:, 2]
        return pos[:, :2], yaw_of(q), q

    # ---- geometry_msgs/Twist
    def twist(self, msg):
        """-> (v m/s along x, w rad/s about z counter-clockwise, the four other components)"""
        lin, ang = msg["linear"], msg["angular"]
        w = -float(ang[2]) if self.misread == "angular.z negated" else float(ang[2])
        return float(lin[0]), w, (float(lin[1]), float(lin[2]), float(ang[0]), float(ang[1]))

    # ---- sensor_msgs/PointCloud2
    def cloud(self, msg):
        """-> float64 (height, width, 3): X, Y, Z of every point by the message's own fields"""
        h, w, ps, rs = (int(msg[k]) for k in ("height", "width", "point_step", "row_step"))
        data = np.frombuffer(bytes(msg["data"]), np.uint8)
        assert data.size >= (h - 1) * rs + (w - 1) * ps + 1 and rs >= w * ps, (data.size, h, w, ps, rs)
        fields = {name: (int(off), int(dt), int(n)) for name, off, dt, n in msg["fields"]}
        out = np.empty((h, w, 3))
        names = ("y", "x", "z") if self.misread == "cloud X and Y swapped" else ("x", "y", "z")
        for axis, name in enumerate(names):
            off, dt, n = fields[name]
            kind = np.dtype((">" if msg["is_bigendian"] else "<") + _FIELD_TYPES[dt])
            assert n == 1 and off + kind.itemsize <= ps, (name, off, dt, n)
            at = (np.arange(h)[:, None] * rs + np.arange(w)[None, :] * ps + off)[..., None] + np.arange(kind.itemsize)
            out[..., axis] = data[at].copy().view(kind)[..., 0]
        return out


# ---- what scene_harness recorded ---------------------------------------------------------------------------------------------------
_GRIDS = ("grid", "costmap", "inflated")
KINDS = _GRIDS + ("scan", "plan", "local_plan", "cmd", "cloud")


def _stamp(text):
    sec, nanosec = text.split(".")
    return int(sec), int(nanosec)


def _f32_text(text):
    """a float32 field, which the harness prints with the nine digits that give the float32 back -> that float32, widened"""
    return float(np.float32(text))


def load_recording(stdout: str, prefix: str) -> dict:
    """scene_harness' lines and files -> {kind: [message, ...] in the order of arrival, "order": [kind, ...]}"""
    out = {k: [] for k in KINDS}
    out["order"] = []
    for line in stdout.splitlines():
        kind = line.split(" ", 1)[0]
        if kind not in KINDS:
            continue
        kv = dict(m.groups() for m in re.finditer(r"(\w+)=(\S*)", line))
        path = f"{prefix}.{kv['seq']}.{kind}"
        m = {}
        if "frame_id" in kv:
            m.update(frame_id=kv["frame_id"], stamp=_stamp(kv["stamp"]))
        if kind in _GRIDS:
            m.update(load=_stamp(kv["load"]), resolution=_f32_text(kv["resolution"]), width=int(kv["width"]), height=int(kv["height"]),
                     origin=tuple(float(v) for v in kv["origin"].split(",")), data=np.fromfile(path, np.int8))
            assert m["data"].size == int(kv["len"])
        elif kind == "scan":
            m.update({k: _f32_text(kv[k]) for k in ("angle_min", "angle_max", "angle_increment", "time_increment", "scan_time", "range_min", "range_max")})
            m.update(ranges=np.fromfile(path, np.float32), intensities=int(kv["intensities"]))
            assert m["ranges"].size == int(kv["ranges"])
        elif kind in ("plan", "local_plan"):
            rows = [l.split(" ") for l in open(path).read().splitlines()]
            assert len(rows) == int(kv["poses"]) and all(len(r) == 10 for r in rows)
            m.update(pose_frame_ids=[r[0] for r in rows], pose_stamps=[(int(r[1]), int(r[2])) for r in rows],
                     positions=np.array([[float(v) for v in r[3:6]] for r in rows], np.float64).reshape(-1, 3),
                     orientations=np.array([[float(v) for v in r[6:10]] for r in rows], np.float64).reshape(-1, 4))
        elif kind == "cmd":
            m.update(linear=tuple(float(kv[k]) for k in ("lx", "ly", "lz")), angular=tuple(float(kv[k]) for k in ("ax", "ay", "az")))
        else:
            m.update({k: int(kv[k]) for k in ("height", "width", "point_step", "row_step")}, is_dense=kv["is_dense"] == "1",
                     is_bigendian=kv["is_bigendian"] == "1", data=np.fromfile(path, np.uint8),
                     fields=[(n, int(o), int(d), int(c)) for n, o, d, c in (f.split(":") for f in kv["fields"].split(",") if f)])
            assert m["data"].size == int(kv["len"])
        out[kind].append(m)
        out["order"].append(kind)
    return out


# ---- what a correct node publishes ---------------------------------------------------------------------------------------------------
def _f32(v):
    return np.float32(v)


def grid_value_of_cost(cost) -> np.ndarray:
    """sn_inflate_grid's documented translation of its cost to a grid value: 0 -> 0, 253 -> 99, 254 -> 100, 255 -> -1, otherwise
    1 + 97 * (cost - 1) / 251 in integers"""
    c = np.asarray(cost).astype(np.int64)
    return np.where(c == 0, 0, np.where(c == 253, 99, np.where(c == 254, 100, np.where(c == 255, -1, 1 + 97 * (c - 1) // 251)))).astype(np.int8)


def lattice(rp):
    """sn_rollout_tables' velocities in double, the parameters as the fp32 the file's text becomes: (v (nv,), w (nw,))"""
    def axis(lo, hi, n):
        lo, hi = float(_f32(lo)), float(_f32(hi))
        return np.array([lo]) if n == 1 else lo + np.arange(n) * ((hi - lo) / (n - 1))
    return axis(rp.v_min, rp.v_max, rp.nv), axis(rp.w_min, rp.w_max, rp.nw)


def cloud_points(raw, cam, out_scale):
    """sn_pointcloud_from_raw's documented arithmetic at step 1 -> float32 (H, W, 3), NaN where the sample is not valid"""
    raw = np.asarray(raw, np.int32)
    h, w = raw.shape
    fx, fy, cx, cy, base = (_f32(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.baseline_mm))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (np.float64(fx * base) / ((raw.astype(np.float32) * _f32(out_scale)).astype(np.float64) * 16.0 * 12.0) / 1000.0).astype(np.float32)
        u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
        x, y = (u - cx) * z / fx, (v - cy) * z / fy
    valid = (raw > 0) & (z >= _f32(cam.z_min_m)) & ((cam.z_max_m <= 0) | (z <= _f32(cam.z_max_m)))
    return np.where(valid[..., None], np.stack([x, y, z], -1), np.float32(np.nan)).astype(np.float32)


def messages_from_chain(R, scene, params) -> dict:
    """What a correct node publishes for a chain's result R (the dict tests/test_chain_truth.py::run_chain returns): the obstacle
    grid, the scan, the costmap and the cloud of every frame, and the inflated grid, the plan, the command and the local plan
    of the last (the chain plans once, at the end of the clip).  params has op, cp, rp (the parameter dataclasses), cam and
    out_scale."""
    op, cp, rp, cam = params.op, params.cp, params.rp, params.cam
    cell = _f32(op.cell_m)
    n = len(scene.poses)
    out = {k: [] for k in KINDS}

    def header(k, frame_id):
        return dict(frame_id=frame_id, stamp=(STAMP_SEC, STAMP_NANOSEC + k))
    for k in range(n):
        stamp = (STAMP_SEC, STAMP_NANOSEC + k)
        # the base-frame grid: cell (ix, iy) covers [x_min + ix * cell, + cell) x [y_min + iy * cell, + cell), data index iy * gw + ix
        out["grid"].append(dict(header(k, op.frame), load=stamp, resolution=float(cell), width=op.gw, height=op.gh,
                                origin=(float(_f32(op.x_min_m)), float(_f32(op.y_min_m)), 0.0, 0.0, 0.0, 0.0, 1.0), data=np.asarray(R["occ"][k], np.int8).reshape(-1)))
        # beam b covers [angle_min + b * increment, + increment): it looks along the middle of that
        a0, da = _f32(op.angle_min_rad), _f32(op.angle_increment_rad)
        first = _f32(a0 + _f32(0.5) * da)
        out["scan"].append(dict(header(k, op.frame), angle_min=float(first), angle_increment=float(da), angle_max=float(_f32(first + _f32(op.beams - 1) * da)),
                                time_increment=0.0, scan_time=0.0, range_min=float(_f32(op.range_min_m)), range_max=float(_f32(op.range_max_m)),
                                ranges=np.asarray(R["ranges"][k], np.float32), intensities=0))
        # the window: element [cy - oy][cx - ox] is world cell (cx, cy), which covers [cx * cell, + cell) x [cy * cell, + cell)
        ox, oy = float(R["q"][k][4]) * float(cell), float(R["q"][k][5]) * float(cell)
        out["costmap"].append(dict(header(k, cp.frame), load=stamp, resolution=float(cell), width=cp.mw, height=cp.mh,
                                   origin=(ox, oy, 0.0, 0.0, 0.0, 0.0, 1.0), data=np.asarray(R["grid"][k], np.int8).reshape(-1)))
        pts = cloud_points(R["raws"][k], cam, params.out_scale)
        cloud = np.zeros(pts.shape[:2] + (4,), np.float32)
        cloud[..., :3] = pts
        cloud.view(np.uint32)[..., 3] = np.where(np.isfinite(pts[..., 2]), 0x808080, 0)      # a grey left eye
        h, w = pts.shape[:2]
        out["cloud"].append(dict(header(k, str(FRAME_INDEX + k)), height=h, width=w, point_step=16, row_step=16 * w, is_dense=False, is_bigendian=False,
                                 fields=[("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 8, 7, 1), ("rgb", 12, 7, 1)], data=cloud.reshape(-1).view(np.uint8)))
    src = out["costmap"][-1]
    out["inflated"].append(dict(src, data=grid_value_of_cost(R["cost"]).reshape(-1)))
    ox, oy, res = src["origin"][0], src["origin"][1], src["resolution"]
    head = dict(frame_id=src["frame_id"], stamp=src["stamp"])

    def path(xy, quats):
        m = len(xy)
        return dict(head, pose_frame_ids=[head["frame_id"]] * m, pose_stamps=[head["stamp"]] * m,
                    positions=np.concatenate([xy, np.zeros((m, 1))], 1).reshape(-1, 3), orientations=np.asarray(quats, np.float64).reshape(-1, 4))
    # one pose per cell of the path at the cell's centre, start first
    cells = np.asarray(R["path"][:int(R["nav_stats"][2])], np.float64).reshape(-1, 2)
    out["plan"].append(path(np.stack([ox + (cells[:, 0] + 0.5) * res, oy + (cells[:, 1] + 0.5) * res], -1), [(0.0, 0.0, 0.0, 1.0)] * len(cells)))
    # the best sample's velocity, and its centre per step: grid coordinates in 1/256 cell, the heading in 1/65536 turn
    if int(R["best"][0]) & 1:
        out["cmd"].append(dict(linear=(0.0, 0.0, 0.0), angular=(0.0, 0.0, 0.0)))
        out["local_plan"].append(path(np.zeros((0, 2)), np.zeros((0, 4))))
    else:
        v, w = lattice(rp)
        iv, iw = divmod(int(R["best"][1]), rp.nw)
        out["cmd"].append(dict(linear=(float(v[iv]), 0.0, 0.0), angular=(0.0, 0.0, float(w[iw]))))
        traj = np.asarray(R["traj"], np.float64)
        half = traj[:, 2] / 65536.0 * math.pi
        zeros = np.zeros(len(half))
        out["local_plan"].append(path(np.stack([ox + traj[:, 0] / 256.0 * res, oy + traj[:, 1] / 256.0 * res], -1),
                                      np.stack([zeros, zeros, np.sin(half), np.cos(half)], -1)))
    out["order"] = None
    return out
