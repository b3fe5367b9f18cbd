"""An analytic terrain and its truth, in float64 and plain numpy: what the elevation map and its traversability verdict are held
to in metres (tests/test_terrain_truth.py, tests/test_gpu_terrain_truth.py), in the spirit of scene_truth.py.

Nothing here is shared with a twin: of the package only ``spec.OUT_SCALE`` and the ``Camera`` dataclass are imported, and the one
relation taken from the product is the documented depth relation of the map, Z_m = fx * baseline_mm / (d * 192 * 1000) with
d = raw * out_scale.  That relation is the sensor model.

The world.  The ground is piecewise planar: a patch is a rectangle [x0, x1] x [y0, y1] over which z = z0 + gx * (x - x0), a
horizontal platform (gx = 0) or a ramp that rises along x.  Patches do not overlap.  A face is a vertical rectangle over the 2-D
segment (x0, y0) - (x1, y1) between the heights zlo and zhi: the riser of a kerb, the wall of a drop, a wall standing on the
floor.  A pose is world (x, y, yaw) on the floor z = 0, yaw counter-clockwise seen from above; the base frame has x forward, y
left, z up.  The camera sits ``cam_height`` above the base origin and looks along base x, pitched down by ``pitch``; its own
frame is X right, Y down, Z forward, so a pixel (u, v) looks along ((u - cx) / fx, (v - cy) / fy, 1) and the depth Z of a hit is
the ray's parameter.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import numpy as np

from hobot_stereonet_amd.pointcloud import Camera
from hobot_stereonet_amd.spec import OUT_SCALE

W, H = 96, 64
CAM = Camera(fx=80.0, fy=80.0, cx=47.5, cy=20.5, baseline_mm=120.0)      # cx = (W - 1) / 2: the mirrored world's image is the mirror image
NONE, GROUND, FACE = 0, 1, 2


@dataclasses.dataclass(frozen=True)
class Terrain:
    """patches: (x0, y0, x1, y1, z0, gx); faces: (x0, y0, x1, y1, zlo, zhi); poses: the clip, the last one is where the robot
    plans from; goal: world (x, y) or None; ramp: the (x0, x1) of the patch that is the ramp, or None; edge_x: the line x =
    edge_x across the way that the robot must not cross (a drop, a kerb), or None; window: the map's (mw, mh)."""
    name: str
    patches: Tuple[Tuple[float, float, float, float, float, float], ...]
    faces: Tuple[Tuple[float, float, float, float, float, float], ...]
    poses: Tuple[Tuple[float, float, float], ...]
    goal: Optional[Tuple[float, float]] = None
    ramp: Optional[Tuple[float, float]] = None
    edge_x: Optional[float] = None
    window: Tuple[int, int] = (80, 64)
    cam_height: float = 0.5
    pitch: float = 0.0


def mirrored(t: Terrain) -> Terrain:
    """the same world with y -> -y and yaw -> -yaw"""
    return dataclasses.replace(
        t, name=t.name + " mirrored", patches=tuple((x0, -y1, x1, -y0, z0, gx) for x0, y0, x1, y1, z0, gx in t.patches),
        faces=tuple((x0, -y0, x1, -y1, zl, zh) for x0, y0, x1, y1, zl, zh in t.faces), poses=tuple((x, -y, -a) for x, y, a in t.poses),
        goal=None if t.goal is None else (t.goal[0], -t.goal[1]))


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------
# the clip ends on ground that its first frames saw (the nearest ground in view is 0.94 m ahead of a level camera 0.5 m up)
_APPROACH = ((0.05, 0.0, 0.0), (0.35, 0.2, -0.15), (0.65, -0.2, 0.2), (0.95, 0.1, -0.25), (1.25, -0.15, 0.1))
_FAR = 9.0
RAMP_TAN = math.tan(math.radians(7.0))
RAMP_TOP = 1.2 * RAMP_TAN                      # 0.1473 m

# Every face lies through the middle of a row of cells, not on a border between two: a cell that holds a face then holds ground on
# both sides of it.
# (a) scene_truth's "free end" as a terrain, half a cell on: a flat floor, and a wall 1.2 m high across the way at x = 3.05 m whose
# free end is at y = 0.45 m
FLAT_WALL = Terrain(name="flat and wall", patches=((-4.0, -6.0, _FAR, 6.0, 0.0, 0.0),), faces=((3.05, 0.45, 3.05, -4.5, 0.0, 1.2),), poses=_APPROACH)
# (b) a ramp of 7 degrees over the whole width from x = 1.8 m to x = 3.0 m, flat before and after: the robot can drive it
RAMP = Terrain(name="ramp", patches=((-4.0, -6.0, 1.8, 6.0, 0.0, 0.0), (1.8, -6.0, 3.0, 6.0, 0.0, RAMP_TAN), (3.0, -6.0, _FAR, 6.0, RAMP_TOP, 0.0)),
               faces=(), poses=_APPROACH, goal=(3.65, 0.15), ramp=(1.8, 3.0))
# (c) a platform that ends at x = 2.55 m in a drop of 0.3 m, the lower floor visible beyond, under a camera pitched down by 0.3 rad
DROP = Terrain(name="drop", patches=((-4.0, -6.0, 2.55, 6.0, 0.0, 0.0), (2.55, -6.0, _FAR, 6.0, -0.3, 0.0)), faces=((2.55, -6.0, 2.55, 6.0, -0.3, 0.0),),
               poses=_APPROACH, goal=(4.05, 0.15), edge_x=2.55, pitch=0.3)
# (d) a kerb of 6 cm across the way at x = 2.25 m
KERB = Terrain(name="kerb", patches=((-4.0, -6.0, 2.25, 6.0, 0.0, 0.0), (2.25, -6.0, _FAR, 6.0, 0.06, 0.0)), faces=((2.25, -6.0, 2.25, 6.0, 0.0, 0.06),),
               poses=_APPROACH, goal=(3.65, 0.15), edge_x=2.25)

BASE = (FLAT_WALL, RAMP, DROP, KERB)
SCENES = {t.name: t for t in BASE}
SCENES.update({t.name: t for t in [mirrored(v) for v in BASE]})


# ---- the terrain as a function -----------------------------------------------------------------------------------------------------------
def height(t: Terrain, xy) -> np.ndarray:
    """the ground's height at world xy (..., 2); NaN outside every patch.  On a shared border the later patch answers."""
    q = np.asarray(xy, np.float64)
    out = np.full(q.shape[:-1], np.nan)
    for x0, y0, x1, y1, z0, gx in t.patches:
        inside = (q[..., 0] >= x0) & (q[..., 0] <= x1) & (q[..., 1] >= y0) & (q[..., 1] <= y1)
        out = np.where(inside, z0 + gx * (q[..., 0] - x0), out)
    return out


def height_range(t: Terrain, lo_xy, hi_xy, z_cap: float = math.inf):
    """the lowest and the highest point of the terrain, faces included (cut at z_cap), over every rectangle [lo_xy, hi_xy]
    (..., 2) -> (zmin, zmax); NaN where the rectangle meets no patch"""
    lo, hi = np.asarray(lo_xy, np.float64), np.asarray(hi_xy, np.float64)
    zmin, zmax = np.full(lo.shape[:-1], np.inf), np.full(lo.shape[:-1], -np.inf)
    for x0, y0, x1, y1, z0, gx in t.patches:
        ax, bx = np.maximum(lo[..., 0], x0), np.minimum(hi[..., 0], x1)
        meets = (ax <= bx) & (np.maximum(lo[..., 1], y0) <= np.minimum(hi[..., 1], y1))
        za, zb = z0 + gx * (ax - x0), z0 + gx * (bx - x0)
        zmin = np.where(meets, np.minimum(zmin, np.minimum(za, zb)), zmin)
        zmax = np.where(meets, np.maximum(zmax, np.maximum(za, zb)), zmax)
    for x0, y0, x1, y1, zl, zh in t.faces:
        meets = (np.maximum(lo[..., 0], min(x0, x1)) <= np.minimum(hi[..., 0], max(x0, x1))) & \
                (np.maximum(lo[..., 1], min(y0, y1)) <= np.minimum(hi[..., 1], max(y0, y1)))      # the faces here run along x or along y
        zmin = np.where(meets, np.minimum(zmin, zl), zmin)
        zmax = np.where(meets, np.maximum(zmax, min(zh, z_cap)), zmax)
    none = ~np.isfinite(zmin)
    return np.where(none, np.nan, zmin), np.where(none, np.nan, zmax)


def face_segments(t: Terrain, min_height: float = 0.0) -> np.ndarray:
    """the faces higher than min_height -> float64 (m, 4) = x0, y0, x1, y1"""
    return np.asarray([f[:4] for f in t.faces if f[5] - f[4] > min_height], np.float64).reshape(-1, 4)


# ---- the sensor --------------------------------------------------------------------------------------------------------------------
def camera_rays(t: Terrain, pose, cam: Camera = CAM, w: int = W, h: int = H):
    """-> (origin float64 (3,), directions float64 (h, w, 3)): the camera's position and every pixel's ray in the world, scaled so
    that the ray's parameter is the depth Z"""
    x, y, yaw = (float(v) for v in pose)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    xc, yc = (u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy                       # camera frame: X right, Y down, Z = 1 forward
    fwd, left, up = np.ones_like(xc), -xc, -yc                                   # level base frame: x forward, y left, z up
    cp, sp = math.cos(t.pitch), math.sin(t.pitch)
    bx, bz = cp * fwd + sp * up, -sp * fwd + cp * up                             # pitched down: forward tips towards -z
    cy_, sy_ = math.cos(yaw), math.sin(yaw)
    d = np.stack([cy_ * bx - sy_ * left, sy_ * bx + cy_ * left, bz], -1)
    return np.array([x, y, t.cam_height]), d


def hit_points(t: Terrain, pose, cam: Camera = CAM, w: int = W, h: int = H):
    """-> (points float64 (h, w, 3) world, NaN without a hit; label uint8 (h, w): NONE, GROUND or FACE; depth float64 (h, w), inf
    without a hit): the nearest of the patches and the faces along every pixel's ray"""
    o, d = camera_rays(t, pose, cam, w, h)
    best = np.full(d.shape[:2], np.inf)
    label = np.zeros(d.shape[:2], np.uint8)
    with np.errstate(divide="ignore", invalid="ignore"):
        for x0, y0, x1, y1, z0, gx in t.patches:
            den = d[..., 2] - gx * d[..., 0]
            ts = (z0 + gx * (o[0] - x0) - o[2]) / den
            px, py = o[0] + ts * d[..., 0], o[1] + ts * d[..., 1]
            ok = (den < 0) & (ts > 0) & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1) & (ts < best)      # den < 0: seen from above
            best, label = np.where(ok, ts, best), np.where(ok, GROUND, label).astype(np.uint8)
        for x0, y0, x1, y1, zl, zh in t.faces:
            ex, ey = x1 - x0, y1 - y0
            den = d[..., 0] * ey - d[..., 1] * ex
            ts = ((x0 - o[0]) * ey - (y0 - o[1]) * ex) / den
            s = ((x0 - o[0]) * d[..., 1] - (y0 - o[1]) * d[..., 0]) / den
            z = o[2] + ts * d[..., 2]
            ok = (den != 0) & (ts > 0) & (s >= 0) & (s <= 1) & (z >= zl) & (z <= zh) & (ts < best)
            best, label = np.where(ok, ts, best), np.where(ok, FACE, label).astype(np.uint8)
    pts = o + np.where(np.isfinite(best), best, np.nan)[..., None] * d
    return pts, label, best


def raw_of_depth(z, cam: Camera = CAM, out_scale: float = OUT_SCALE) -> np.ndarray:
    """the map's integer of a depth in metres, by the documented relation alone; 0 without a hit"""
    with np.errstate(divide="ignore"):
        d = cam.fx * cam.baseline_mm / (np.asarray(z, np.float64) * 192.0 * 1000.0)
    return np.where(np.isfinite(z), np.rint(d / out_scale), 0).astype(np.int32)


def render(t: Terrain, pose, cam: Camera = CAM, w: int = W, h: int = H, out_scale: float = OUT_SCALE) -> np.ndarray:
    """-> raw int32 (h, w): one ray per pixel, the nearest of patches and faces, its depth turned into the map's integer"""
    return raw_of_depth(hit_points(t, pose, cam, w, h)[2], cam, out_scale)


def depth_half_step(z, cam: Camera = CAM, out_scale: float = OUT_SCALE):
    """how far half a unit of the map's integer moves a depth of z metres: Z^2 * 192000 / (fx * baseline_mm) * out_scale / 2"""
    return np.asarray(z, np.float64) ** 2 * 192000.0 / (cam.fx * cam.baseline_mm) * out_scale / 2.0


def mount(t: Terrain) -> Tuple[float, ...]:
    """base_from_cam of the terrain's camera, written out from the frames above: x = cp Z - sp Y, y = -X, z = -sp Z - cp Y + h"""
    cp, sp = math.cos(t.pitch), math.sin(t.pitch)
    return (0.0, -sp, cp, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, -cp, -sp, t.cam_height)


# ---- frames --------------------------------------------------------------------------------------------------------------------------
def to_base(pose, xy) -> np.ndarray:
    """world points (..., 2) in the base frame of a pose"""
    x, y, yaw = (float(v) for v in pose)
    p = np.asarray(xy, np.float64) - (x, y)
    c, s = math.cos(yaw), math.sin(yaw)
    return np.stack([c * p[..., 0] + s * p[..., 1], -s * p[..., 0] + c * p[..., 1]], -1)


def window_origin(pose, cell: float, mw: int, mh: int) -> Tuple[int, int]:
    """the world cell that the rolling window's element [0][0] holds when it is centred on a pose"""
    return int(math.floor(pose[0] / cell)) - mw // 2, int(math.floor(pose[1] / cell)) - mh // 2


def cell_centres(origin, cell: float, mw: int, mh: int) -> np.ndarray:
    """world xy of the centre of every cell of a window -> float64 (mh, mw, 2): element [j][i] is world cell (ox + i, oy + j)"""
    i, j = np.meshgrid(np.arange(mw), np.arange(mh))
    return np.stack([(origin[0] + i + 0.5) * cell, (origin[1] + j + 0.5) * cell], -1)


def dist_to_segments(segs, xy) -> np.ndarray:
    """the exact Euclidean distance of every xy (..., 2) to the nearest of the segments (k, 4); inf for an empty set"""
    q = np.asarray(xy, np.float64).reshape(-1, 1, 2)
    a = np.asarray(segs, np.float64).reshape(-1, 4)
    if not len(a):
        return np.full(np.shape(xy)[:-1], np.inf)
    p0, e = a[None, :, 0:2], a[None, :, 2:4] - a[None, :, 0:2]
    s = np.clip(((q - p0) * e).sum(-1) / np.maximum((e * e).sum(-1), 1e-300), 0.0, 1.0)
    return np.sqrt(((q - (p0 + s[..., None] * e)) ** 2).sum(-1).min(1)).reshape(np.shape(xy)[:-1])


def frame_rays(t: Terrain, pose, cell: float, range_max: float, z_band, margin: float):
    """The rays of one frame that the map may use -> (world cell int64 (k, 2), height float64 (k,), depth float64 (k,), sure bool
    (k,), candidates int64 (k, 4, 2)): hits within range_max + margin of the base origin and with a height inside z_band widened
    by margin.  sure: the hit keeps `margin` from its cell's borders, from range_max and from the band's ends, so it counts in
    that cell whatever the roundings of the map do.  candidates: the cells the hit may count in when it is moved by up to
    `margin` along x and y (the four corners' cells, repeated where they agree)."""
    pts, label, depth = hit_points(t, pose)
    sel = label != NONE
    p, zd = pts[sel], depth[sel]
    r = np.hypot(*to_base(pose, p[:, :2]).T)
    keep = (r <= range_max + margin) & (p[:, 2] >= z_band[0] - margin) & (p[:, 2] <= z_band[1] + margin)
    p, zd, r = p[keep], zd[keep], r[keep]
    f = p[:, :2] / cell
    c = np.floor(f).astype(np.int64)
    frac = np.minimum(f - c, c + 1 - f).min(1) * cell
    sure = (frac > margin) & (r <= range_max - margin) & (p[:, 2] >= z_band[0] + margin) & (p[:, 2] <= z_band[1] - margin)
    corners = np.stack([p[:, :2] + (sx * margin, sy * margin) for sx in (-1, 1) for sy in (-1, 1)], 1)
    return c, p[:, 2], zd, sure, np.floor(corners / cell).astype(np.int64)
