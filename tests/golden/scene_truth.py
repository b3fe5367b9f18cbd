"""An analytic world and its truth, in float64 and plain numpy: what the chain obstacle grid -> costmap -> inflation -> path ->
rollout is held to in metres (tests/test_chain_truth.py, tests/test_gpu_chain_truth.py).

Nothing here is shared with a twin: of the package only ``spec.OUT_SCALE`` and the ``Camera`` dataclass are imported, and the one
relation taken from the product is the documented depth relation of the map, Z_m = fx * baseline_mm / (d * 192 * 1000) with
d = raw * out_scale (what ``sn_depth_from_raw`` is pinned to).  That relation is the sensor model.

The world.  The ground is z = 0.  A wall is a 2-D segment with a height, a box four such segments around an interior no ray
enters.  A pose is world (x, y, yaw), yaw counter-clockwise seen from above.  The base frame has x forward, y left, z up.  The
camera sits ``cam_height`` above the base origin and looks along base x, pitched down by ``pitch`` (its forward axis tips
towards -z); its own frame is X right, Y down, Z forward, so a pixel (u, v) looks along ((u - cx) / fx, (v - cy) / fy, 1) and
the depth Z of a hit is the ray's parameter.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Tuple

import numpy as np

from hobot_stereonet_amd.pointcloud import Camera
from hobot_stereonet_amd.spec import OUT_SCALE

W, H = 96, 64
CAM = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0)      # cx = (W - 1) / 2: the mirrored world's image is the mirror image
NONE, GROUND, WALL = 0, 1, 2


@dataclasses.dataclass(frozen=True)
class Scene:
    """walls: (x0, y0, x1, y1, height); boxes: (x_min, y_min, x_max, y_max, height); poses: the clip, the last one is where the
    robot plans from; goal: world (x, y); gate: the segment on the wall's line that is the true opening; via: the corners of the
    zero-clearance geodesic between the last pose and the goal; witness_via: the inner points of a hand-made polyline from the
    last pose to the goal that keeps wide of every wall; window: the costmap's (mw, mh); left: +1 where the way round is on the
    robot's left, -1 on its right, 0 where the scene does not say."""
    name: str
    walls: Tuple[Tuple[float, float, float, float, float], ...]
    boxes: Tuple[Tuple[float, float, float, float, float], ...]
    poses: Tuple[Tuple[float, float, float], ...]
    goal: Tuple[float, float]
    gate: Tuple[Tuple[float, float], Tuple[float, float]]
    via: Tuple[Tuple[float, float], ...]
    witness_via: Tuple[Tuple[float, float], ...]
    window: Tuple[int, int] = (100, 100)
    cam_height: float = 0.5
    pitch: float = 0.0
    left: int = 0
    fitted_mount: bool = False


def segments(scene: Scene) -> np.ndarray:
    """every vertical face of the scene -> float64 (m, 5) = x0, y0, x1, y1, height"""
    out = [list(w) for w in scene.walls]
    for x0, y0, x1, y1, h in scene.boxes:
        out += [[x0, y0, x1, y0, h], [x1, y0, x1, y1, h], [x1, y1, x0, y1, h], [x0, y1, x0, y0, h]]
    return np.asarray(out, np.float64).reshape(-1, 5)


def mirrored(scene: Scene) -> Scene:
    """the same world with y -> -y and yaw -> -yaw"""
    fy = lambda pts: tuple((x, -y) for x, y in pts)      # noqa: E731
    return dataclasses.replace(
        scene, name=scene.name + " mirrored", walls=tuple((x0, -y0, x1, -y1, h) for x0, y0, x1, y1, h in scene.walls),
        boxes=tuple((x0, -y1, x1, -y0, h) for x0, y0, x1, y1, h in scene.boxes), poses=tuple((x, -y, -a) for x, y, a in scene.poses),
        goal=(scene.goal[0], -scene.goal[1]), gate=fy(scene.gate), via=fy(scene.via), witness_via=fy(scene.witness_via), left=-scene.left)


# ---- the four scenes ---------------------------------------------------------------------------------------------------------------
_APPROACH = ((0.05, 0.0, 0.0), (0.35, 0.2, -0.15), (0.65, -0.2, 0.2), (0.95, 0.1, -0.25), (1.25, -0.4, 0.3), (1.45, -0.1, -0.1), (1.65, -0.35, 0.15))      # ends on a cell's centre, as every goal does

# 1: one wall across the way at x = 3 m whose free end is at y = 0.4 m: the only way round is on the left
FREE_END = Scene(name="free end", walls=((3.0, 0.4, 3.0, -4.5, 1.2),), boxes=(), poses=_APPROACH, goal=(4.65, -0.65),
                 gate=((3.0, 0.4), (3.0, 4.5)), via=((3.0, 0.4),), witness_via=((1.9, 1.0), (2.4, 1.5), (3.6, 1.5), (4.1, 1.0)), left=1)
# 2: a wall with a gap of 2.2 m around y = 0.2 and a box behind the gap
GAP = Scene(name="gap and box", walls=((3.0, -0.9, 3.0, -4.5, 1.2), (3.0, 1.3, 3.0, 4.5, 1.2)), boxes=((4.4, -0.9, 4.9, -0.3, 0.9),),
            poses=_APPROACH, goal=(5.35, 1.65), gate=((3.0, -0.9), (3.0, 1.3)), via=(), witness_via=((2.0, 0.2), (3.4, 0.2), (4.3, 1.0)))
# 3: a corridor 2.2 m wide that turns left by 90 degrees, driven along and then backed out of by two frames (the camera keeps
# looking along +y): the window of 64 cells re-centres by 42 cells in y and then comes 12 back
_DRIVE = ((0.0, 0.0, 0.0), (0.6, 0.0, 0.0), (1.2, 0.0, 0.1), (1.8, 0.05, 0.3), (2.4, 0.3, 0.7), (2.8, 0.8, 1.1), (3.0, 1.4, 1.45),
          (3.05, 2.2, math.pi / 2), (3.05, 3.2, math.pi / 2), (3.05, 4.25, math.pi / 2), (3.05, 3.65, math.pi / 2), (3.05, 3.05, math.pi / 2))
CORRIDOR = Scene(name="corridor", walls=((-1.0, -1.2, 4.2, -1.2, 1.2), (4.2, -1.2, 4.2, 9.0, 1.2), (-1.0, 1.0, 2.0, 1.0, 1.2), (2.0, 1.0, 2.0, 9.0, 1.2)),
                 boxes=(), poses=_DRIVE, goal=(3.05, 5.65), gate=((2.0, 4.5), (4.2, 4.5)), via=(), witness_via=(), window=(64, 64))
# 4: scene 1 under a camera pitched down by 0.2 rad, whose mount the chain takes from the ground fit frame by frame
PITCHED = dataclasses.replace(FREE_END, name="free end pitched", pitch=0.2, fitted_mount=True)

SCENES = {s.name: s for s in (FREE_END, GAP, CORRIDOR, PITCHED)}
SCENES.update({s.name: s for s in [mirrored(v) for v in (FREE_END, GAP, CORRIDOR, PITCHED)]})


# ---- the sensor --------------------------------------------------------------------------------------------------------------------
def camera_rays(scene: Scene, pose, cam: Camera = CAM, w: int = W, h: int = H):
    """-> (origin float64 (3,), directions float64 (h, w, 3)): the camera's position and every pixel's ray in the world, scaled so
    that the ray's parameter is the depth Z"""
    x, y, yaw = (float(v) for v in pose)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    xc, yc = (u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy                       # camera frame: X right, Y down, Z = 1 forward
    fwd, left, up = np.ones_like(xc), -xc, -yc                                   # level base frame: x forward, y left, z up
    cp, sp = math.cos(scene.pitch), math.sin(scene.pitch)
    bx, bz = cp * fwd + sp * up, -sp * fwd + cp * up                             # pitched down: forward tips towards -z
    cy_, sy_ = math.cos(yaw), math.sin(yaw)
    d = np.stack([cy_ * bx - sy_ * left, sy_ * bx + cy_ * left, bz], -1)
    return np.array([x, y, scene.cam_height]), d


def hit_points(scene: Scene, pose, cam: Camera = CAM, w: int = W, h: int = H):
    """-> (points float64 (h, w, 3) world, NaN without a hit; label uint8 (h, w): NONE, GROUND or WALL; depth float64 (h, w), inf
    without a hit): the nearest of the ground and the vertical faces along every pixel's ray"""
    o, d = camera_rays(scene, pose, cam, w, h)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d[..., 2] < 0, -o[2] / d[..., 2], np.inf)
        label = np.where(np.isfinite(t), GROUND, NONE).astype(np.uint8)
        for x0, y0, x1, y1, hgt in segments(scene):
            ex, ey = x1 - x0, y1 - y0
            den = d[..., 0] * ey - d[..., 1] * ex
            ts = ((x0 - o[0]) * ey - (y0 - o[1]) * ex) / den                     # o + ts * d = p0 + s * e
            s = ((x0 - o[0]) * d[..., 1] - (y0 - o[1]) * d[..., 0]) / den
            z = o[2] + ts * d[..., 2]
            ok = (den != 0) & (ts > 0) & (s >= 0) & (s <= 1) & (z >= 0) & (z <= hgt) & (ts < t)
            t = np.where(ok, ts, t)
            label = np.where(ok, WALL, label).astype(np.uint8)
    pts = o + np.where(np.isfinite(t), t, np.nan)[..., None] * d
    return pts, label, t


def raw_of_depth(z, cam: Camera = CAM, out_scale: float = OUT_SCALE) -> np.ndarray:
    """the map's integer of a depth in metres, by the documented relation alone; 0 without a hit"""
    with np.errstate(divide="ignore"):
        d = cam.fx * cam.baseline_mm / (np.asarray(z, np.float64) * 192.0 * 1000.0)
    return np.where(np.isfinite(z), np.rint(d / out_scale), 0).astype(np.int32)


def render(scene: Scene, pose, cam: Camera = CAM, w: int = W, h: int = H, out_scale: float = OUT_SCALE) -> np.ndarray:
    """-> raw int32 (h, w): one ray per pixel, the nearest of ground and walls, its depth turned into the map's integer"""
    return raw_of_depth(hit_points(scene, pose, cam, w, h)[2], cam, out_scale)


def depth_half_step(z: float, cam: Camera = CAM, out_scale: float = OUT_SCALE) -> float:
    """how far half a unit of the map's integer moves a depth of z metres: Z^2 * 192000 / (fx * baseline_mm) * out_scale / 2"""
    return z * z * 192000.0 / (cam.fx * cam.baseline_mm) * out_scale / 2.0


# ---- frames --------------------------------------------------------------------------------------------------------------------------
def to_base(pose, xy) -> np.ndarray:
    """world points (..., 2) in the base frame of a pose"""
    x, y, yaw = (float(v) for v in pose)
    p = np.asarray(xy, np.float64) - (x, y)
    c, s = math.cos(yaw), math.sin(yaw)
    return np.stack([c * p[..., 0] + s * p[..., 1], -s * p[..., 0] + c * p[..., 1]], -1)


def to_world(pose, xy) -> np.ndarray:
    """base-frame points (..., 2) in the world"""
    x, y, yaw = (float(v) for v in pose)
    p = np.asarray(xy, np.float64)
    c, s = math.cos(yaw), math.sin(yaw)
    return np.stack([x + c * p[..., 0] - s * p[..., 1], y + s * p[..., 0] + c * p[..., 1]], -1)


# ---- truth queries -------------------------------------------------------------------------------------------------------------------
def wall_rays(scene: Scene, pose, grid, z_band, edge: float = 0.0):
    """The wall rays of one frame that fall on a base-frame grid = (x_min, y_min, cell, gw, gh) with a height inside z_band =
    (lo, hi] -> (world xyz float64 (k, 3), cell index int64 (k, 2) = (ix, iy), near bool (k,): the point lies within `edge`
    cells of a cell border or of the band's ends), and the depth float64 (k,)"""
    x_min, y_min, cell, gw, gh = grid
    pts, label, depth = hit_points(scene, pose)
    sel = label == WALL
    p, zd = pts[sel], depth[sel]
    b = to_base(pose, p[:, :2])
    fx, fy = (b[:, 0] - x_min) / cell, (b[:, 1] - y_min) / cell
    ix, iy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    keep = (ix >= 0) & (ix < gw) & (iy >= 0) & (iy < gh) & (p[:, 2] > z_band[0]) & (p[:, 2] <= z_band[1])
    frac = np.minimum(np.minimum(fx - ix, ix + 1 - fx), np.minimum(fy - iy, iy + 1 - fy))
    near = (frac < edge) | (np.abs(p[:, 2] - z_band[0]) < edge * cell) | (np.abs(p[:, 2] - z_band[1]) < edge * cell)
    return p[keep], np.stack([ix, iy], 1)[keep], near[keep], zd[keep]


def seen_wall(scene: Scene, poses, min_rays: int, grid, z_band) -> np.ndarray:
    """The wall points that count as seen -> world xy float64 (k, 2): those whose base-frame cell received at least min_rays
    wall rays in one frame"""
    out = []
    gw = grid[3]
    for pose in poses:
        p, idx, _, _ = wall_rays(scene, pose, grid, z_band)
        key = idx[:, 1] * gw + idx[:, 0]
        cells, counts = np.unique(key, return_counts=True)
        out.append(p[np.isin(key, cells[counts >= min_rays]), :2])
    return np.concatenate(out) if out else np.zeros((0, 2))


def dist_to(what, xy, chunk: int = 256) -> np.ndarray:
    """The exact Euclidean distance of every query point xy (..., 2) to the nearest of `what`: points (k, 2), or segments (k, 4+)
    = x0, y0, x1, y1; inf for an empty set"""
    q = np.asarray(xy, np.float64).reshape(-1, 2)
    a = np.asarray(what, np.float64)
    out = np.full(q.shape[0], np.inf)
    if a.shape[0] == 0:
        return out.reshape(np.shape(xy)[:-1])
    for i in range(0, q.shape[0], chunk):
        c = q[i:i + chunk, None, :]
        if a.shape[1] == 2:
            d2 = ((c - a[None]) ** 2).sum(-1)
        else:
            p0, e = a[None, :, 0:2], a[None, :, 2:4] - a[None, :, 0:2]
            s = np.clip(((c - p0) * e).sum(-1) / np.maximum((e * e).sum(-1), 1e-300), 0.0, 1.0)
            d2 = ((c - (p0 + s[..., None] * e)) ** 2).sum(-1)
        out[i:i + chunk] = np.sqrt(d2.min(1))
    return out.reshape(np.shape(xy)[:-1])


def crossing(p, q, a, b):
    """where the segment p -> q properly crosses the segment a -> b: the parameter along p -> q, or None (touching an end of
    either counts as no crossing)"""
    p, q, a, b = (np.asarray(v, np.float64)[:2] for v in (p, q, a, b))
    r, e = q - p, b - a
    den = r[0] * e[1] - r[1] * e[0]
    if den == 0:
        return None
    t = ((a[0] - p[0]) * e[1] - (a[1] - p[1]) * e[0]) / den
    s = ((a[0] - p[0]) * r[1] - (a[1] - p[1]) * r[0]) / den
    return float(t) if 0 < t < 1 and 0 < s < 1 else None


def visible(scene: Scene, pose, xy) -> np.ndarray:
    """2-D: true where the segment from the camera's ground position to xy (..., 2) crosses no vertical face"""
    o = np.asarray(pose, np.float64)[:2]
    q = np.asarray(xy, np.float64)
    r = q - o
    clear = np.ones(q.shape[:-1], bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for x0, y0, x1, y1, _ in segments(scene):
            ex, ey = x1 - x0, y1 - y0
            den = r[..., 0] * ey - r[..., 1] * ex
            t = ((x0 - o[0]) * ey - (y0 - o[1]) * ex) / den
            s = ((x0 - o[0]) * r[..., 1] - (y0 - o[1]) * r[..., 0]) / den
            clear &= ~((den != 0) & (t > 0) & (t < 1) & (s >= 0) & (s <= 1))
    return clear


def arc(pose, v: float, w: float, t):
    """The closed-form unicycle: from pose, at speed v (m/s, along the heading) and turn rate w (rad/s, positive = to the left)
    for t seconds -> (x, y, heading), each of t's shape.  In the robot's own frame the arc is (r sin th, r (1 - cos th)) with
    r = v / w and th = w t; for w -> 0 the straight line (v t, 0) (the limit, taken below |th| = 1e-9 where the closed form
    loses its digits)."""
    x0, y0, yaw = (float(a) for a in pose)
    t = np.asarray(t, np.float64)
    th = w * t
    small = np.abs(th) < 1e-9
    safe = np.where(small, 1.0, th)
    fx = np.where(small, v * t, v * t * np.sin(safe) / safe)
    fy = np.where(small, v * t * th / 2.0, v * t * (1.0 - np.cos(safe)) / safe)
    c, s = math.cos(yaw), math.sin(yaw)
    return x0 + c * fx - s * fy, y0 + s * fx + c * fy, yaw + th


def polyline_length(points) -> float:
    p = np.asarray(points, np.float64).reshape(-1, 2)
    return float(np.sqrt((np.diff(p, axis=0) ** 2).sum(1)).sum())


def witness(scene: Scene) -> np.ndarray:
    """A hand-made polyline from the last pose to the goal -> float64 (k, 2); witness_clearance says how far it keeps from every
    wall, and its length bounds the planner's path from above"""
    return np.asarray([scene.poses[-1][:2], *scene.witness_via, scene.goal], np.float64)


def witness_clearance(scene: Scene, step: float = 0.005) -> float:
    """the smallest distance of the witness, sampled every `step` metres, to any vertical face"""
    p = witness(scene)
    pts = [p[-1:]]
    for a, b in zip(p[:-1], p[1:]):
        k = max(2, int(math.ceil(np.hypot(*(b - a)) / step)))
        pts.append(a + (b - a) * np.linspace(0.0, 1.0, k, endpoint=False)[:, None])
    return float(dist_to(segments(scene), np.concatenate(pts)).min())


def geodesic(scene: Scene) -> np.ndarray:
    """the zero-clearance shortest way from the last pose to the goal: straight but for the corners it bends around"""
    return np.asarray([scene.poses[-1][:2], *scene.via, scene.goal], np.float64)


def crosses_walls(scene: Scene, points) -> bool:
    """true where a polyline crosses a vertical face"""
    p = np.asarray(points, np.float64).reshape(-1, 2)
    return any(crossing(a, b, s[0:2], s[2:4]) is not None for a, b in zip(p[:-1], p[1:]) for s in segments(scene))


def window_origin(pose, cell: float, mw: int, mh: int) -> Tuple[int, int]:
    """the world cell that the rolling window's element [0][0] holds when it is centred on a pose: the pose's cell less half
    the window"""
    return int(math.floor(pose[0] / cell)) - mw // 2, int(math.floor(pose[1] / cell)) - mh // 2


def cell_centres(origin, cell: float, mw: int, mh: int) -> np.ndarray:
    """world xy of the centre of every cell of a window -> float64 (mh, mw, 2): element [j][i] is world cell (ox + i, oy + j)"""
    i, j = np.meshgrid(np.arange(mw), np.arange(mh))
    return np.stack([(origin[0] + i + 0.5) * cell, (origin[1] + j + 0.5) * cell], -1)


def in_view(pose, xy, cam: Camera = CAM, w: int = W, slack: float = 0.0) -> np.ndarray:
    """2-D: true where xy lies ahead of the camera inside the image's horizontal field of view widened by `slack` metres"""
    b = to_base(pose, xy)
    tl, tr = (cam.cx + 0.5) / cam.fx, (w - 0.5 - cam.cx) / cam.fx              # tan of the half angles to the left and right
    return (b[..., 0] > -slack) & (b[..., 1] <= b[..., 0] * tl + slack * math.hypot(1, tl)) & (-b[..., 1] <= b[..., 0] * tr + slack * math.hypot(1, tr))
