"""Bird's-eye obstacle grid and laser scan from the int32 disparity map: the parameters of ``sn_obstacles_from_raw``
(include/stereonet_hip.h), a numpy twin of its arithmetic (bit-exact: every fp32 step rounded as the kernel rounds it, every
accumulator an integer), the parameter file of the tools and the node, and the two files ``filelist --obstacles`` writes.

The point arithmetic has one statement: X, Y, Z and validity are ``pointcloud.reference``'s.  The base frame has x forward,
y left, z up; the camera frame is the point cloud's (X right, Y down, Z forward).
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Tuple

import numpy as np

from . import paramfile, pointcloud, spec

MAX_CELLS = 4096                    # gw, gh
MAX_BEAMS = 4096
INF_BITS = 0x7f800000               # a beam without a return
NO_HEIGHT = -(1 << 31)              # height_mm of a cell without an obstacle point
OCCUPIED, FREE, UNKNOWN = 100, 0, -1
LEVEL_MOUNT = (0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0)      # x = Z, y = -X, z = -Y, t = 0


@dataclasses.dataclass
class ObstacleParams:
    """sn_obstacle_params.  base_from_cam: row-major 3x4 [R|t] in metres, all twelve zero = the level forward mount.  gw = gh
    = 0: no grid; beams = 0: no scan.  frame is the node's frame id (not part of the struct)."""
    base_from_cam: Tuple[float, ...] = (0.0,) * 12
    x_min_m: float = 0.0
    y_min_m: float = -5.0
    cell_m: float = 0.1
    gw: int = 100
    gh: int = 100
    z_floor_m: float = -0.15
    z_lo_m: float = 0.1
    z_hi_m: float = 1.5
    min_obstacle_hits: int = 3
    min_ground_hits: int = 3
    beams: int = 0
    angle_min_rad: float = 0.0
    angle_increment_rad: float = 0.0
    range_min_m: float = 0.0
    range_max_m: float = 0.0
    frame: str = "base_link"

    def matrix(self) -> np.ndarray:
        """the twelve float32 the arithmetic uses"""
        m = np.asarray(self.base_from_cam, np.float32).reshape(12)
        return np.asarray(LEVEL_MOUNT, np.float32) if not m.any() else m


_FLOATS = ("x_min_m", "y_min_m", "cell_m", "z_floor_m", "z_lo_m", "z_hi_m", "angle_min_rad", "angle_increment_rad", "range_min_m",
           "range_max_m")
_INTS = ("gw", "gh", "min_obstacle_hits", "min_ground_hits", "beams")


def mount(yaw_rad: float = 0.0, pitch_down_rad: float = 0.0, t=(0.0, 0.0, 0.0)) -> Tuple[float, ...]:
    """base_from_cam of a camera at t that looks along the base x axis turned by yaw (to the left) and pitched down."""
    cy, sy, cp, sp = np.cos(yaw_rad), np.sin(yaw_rad), np.cos(pitch_down_rad), np.sin(pitch_down_rad)
    level = np.asarray(LEVEL_MOUNT, np.float64).reshape(3, 4)[:, :3]
    pitch = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])          # about the base y axis: forward tips towards -z
    yaw = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    r = yaw @ pitch @ level
    return tuple(float(np.float32(v)) for v in np.concatenate([r, np.asarray(t, np.float64).reshape(3, 1)], axis=1).reshape(12))


def check(p: ObstacleParams) -> Optional[str]:
    """None, or why sn_obstacles_from_raw refuses these parameters (the sector of a scan apart: beam_edges says)."""
    vals = list(np.asarray(p.base_from_cam, np.float64).reshape(-1)) + [getattr(p, k) for k in _FLOATS]
    if len(p.base_from_cam) != 12 or not np.all(np.isfinite(np.asarray(vals, np.float32))):
        return "every parameter must be finite, base_from_cam twelve numbers"
    if not np.float32(p.cell_m) > 0:
        return "cell_m must be positive"
    if p.gw < 0 or p.gh < 0 or p.gw > MAX_CELLS or p.gh > MAX_CELLS or (p.gw == 0) != (p.gh == 0):
        return "gw and gh must be 1..4096, or both 0"
    if p.beams < 0 or p.beams > MAX_BEAMS:
        return "beams must be 0..4096"
    if np.float32(p.z_floor_m) > np.float32(p.z_lo_m) or np.float32(p.z_lo_m) > np.float32(p.z_hi_m):
        return "z_floor_m <= z_lo_m <= z_hi_m is required"
    if p.min_obstacle_hits < 0 or p.min_ground_hits < 0:
        return "the hit thresholds must not be negative"
    if np.float32(p.range_min_m) < 0 or np.float32(p.range_max_m) < np.float32(p.range_min_m):
        return "0 <= range_min_m <= range_max_m is required"
    return None


def beam_edges(p: ObstacleParams) -> np.ndarray:
    """sn_obstacle_beam_edges: float32 (beams + 1,), edges[i] = (float)tan((double)angle_min + (double)i * (double)increment).
    ValueError unless 1 <= beams <= 4096, the sector lies inside (-pi/2, pi/2) and the edges increase strictly."""
    a0, da = np.float64(np.float32(p.angle_min_rad)), np.float64(np.float32(p.angle_increment_rad))
    if p.beams < 1 or p.beams > MAX_BEAMS or not (np.isfinite(a0) and np.isfinite(da)):
        raise ValueError("beams must be 1..4096 and the sector finite")
    a = a0 + np.arange(p.beams + 1, dtype=np.float64) * da
    if not np.all((a > -np.pi / 2) & (a < np.pi / 2)):
        raise ValueError("the sector must lie inside (-pi/2, pi/2)")
    e = np.tan(a).astype(np.float32)
    if not np.all(e[1:] > e[:-1]):
        raise ValueError("the beam edges must increase strictly")
    return e


def beam_angles(p: ObstacleParams) -> np.ndarray:
    """the centre angle of every beam, float64 (beams,): angle_min + (i + 0.5) * increment"""
    return np.float64(np.float32(p.angle_min_rad)) + (np.arange(p.beams) + 0.5) * np.float64(np.float32(p.angle_increment_rad))


def base_points(raw: np.ndarray, cam: pointcloud.Camera, p: ObstacleParams, out_scale: float = spec.OUT_SCALE):
    """-> (xb, yb, zb) float32 (n, Ho, Wo): the base-frame coordinates of every sample, NaN where the sample is not valid."""
    pts, _ = pointcloud.reference(np.asarray(raw, np.int32).reshape((-1,) + np.shape(raw)[-2:]), cam, pointcloud.ORGANISED,
                                  out_scale=out_scale)
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    m = p.matrix()
    with np.errstate(invalid="ignore", over="ignore"):
        return tuple(((m[4 * i] * x + m[4 * i + 1] * y) + m[4 * i + 2] * z) + m[4 * i + 3] for i in range(3))


def reference(raw: np.ndarray, cam: pointcloud.Camera, p: ObstacleParams, edges: Optional[np.ndarray] = None,
              out_scale: float = spec.OUT_SCALE):
    """The header's arithmetic on the host.  raw int32 (H, W) or (n, H, W) -> (occ int8 (n, gh, gw), hits uint32 (n, gh, gw, 2),
    height_mm int32 (n, gh, gw), ranges float32 (n, beams), stats uint32 (n, 4)); leading n dropped when raw is 2-D.  edges:
    the beam table to use (the library's, say) instead of beam_edges(p)."""
    why = check(p)
    if why:
        raise ValueError(why)
    f32 = np.float32
    single = np.ndim(raw) == 2
    xb, yb, zb = base_points(raw, cam, p, out_scale)
    n = xb.shape[0]
    gw, gh, cells = p.gw, p.gh, p.gw * p.gh
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ground = (f32(p.z_floor_m) <= zb) & (zb <= f32(p.z_lo_m))
        obstacle = (f32(p.z_lo_m) < zb) & (zb <= f32(p.z_hi_m))
        hits = np.zeros((n, cells, 2), np.uint32)
        height = np.full((n, cells), NO_HEIGHT, np.int32)
        if cells:
            qx = np.floor((xb - f32(p.x_min_m)) / f32(p.cell_m))
            qy = np.floor((yb - f32(p.y_min_m)) / f32(p.cell_m))
            inside = (qx >= 0) & (qx < f32(gw)) & (qy >= 0) & (qy < f32(gh)) & (ground | obstacle)
            mm = np.clip(np.floor(zb * f32(1000.0)).astype(np.float64), -2.0 ** 31, 2.0 ** 31 - 1)
            for k in range(n):
                sel = inside[k]
                cell = qy[k][sel].astype(np.int64) * gw + qx[k][sel].astype(np.int64)
                ob = obstacle[k][sel]
                hits[k, :, 0] = np.bincount(cell[ob], minlength=cells)
                hits[k, :, 1] = np.bincount(cell[~ob], minlength=cells)
                np.maximum.at(height[k], cell[ob], mm[k][sel][ob].astype(np.int64).astype(np.int32))
        occ = np.where(hits[..., 0] >= p.min_obstacle_hits, OCCUPIED, np.where(hits[..., 1] >= p.min_ground_hits, FREE, UNKNOWN)).astype(np.int8)
        stats = np.stack([hits[..., 0].sum(axis=1), hits[..., 1].sum(axis=1), (occ == OCCUPIED).sum(axis=1), (occ == FREE).sum(axis=1)],
                         axis=1).astype(np.uint32)
        bits = np.full((n, p.beams), INF_BITS, np.uint32)
        if p.beams:
            e = beam_edges(p) if edges is None else np.asarray(edges, f32).reshape(p.beams + 1)
            t = yb / xb
            r = np.sqrt(xb * xb + yb * yb)
            seen = obstacle & (xb > 0) & (e[0] <= t) & (t < e[-1]) & (f32(p.range_min_m) <= r) & (r <= f32(p.range_max_m))
            for k in range(n):
                beam = np.searchsorted(e, t[k][seen[k]], side="right") - 1
                np.minimum.at(bits[k], beam, r[k][seen[k]].view(np.uint32))
    out = (occ.reshape(n, gh, gw), hits.reshape(n, gh, gw, 2), height.reshape(n, gh, gw), bits.view(f32), stats)
    return tuple(a[0] for a in out) if single else out


def ground_and_wall(w: int, h: int, cam: pointcloud.Camera, cam_height_m: float, wall_z_m: float,
                    out_scale: float = spec.OUT_SCALE) -> np.ndarray:
    """A synthetic map, int32 (h, w): a level camera cam_height_m above a ground plane looks at a fronto-parallel wall at
    Z = wall_z_m; every pixel holds the nearer of the two, rounded to the map's integer by out_scale."""
    c = cam.resolved(w, h)
    dv = np.arange(h, dtype=np.float64)[:, None] - c.cy
    zg = np.where(dv > 0, cam_height_m * c.fy / np.where(dv > 0, dv, 1.0), np.inf)
    z = np.broadcast_to(np.minimum(zg, wall_z_m), (h, w))
    return np.rint(c.fx * c.baseline_mm / (z * 1000.0 * 16.0 * 12.0 * out_scale)).astype(np.int32)


# ---- the parameter file: one `key value...` per line, `#` comments, as the calibration file ------------------------------------
_FILE = paramfile.spec(_FLOATS, _INTS, base_from_cam=paramfile.Key(12), frame=paramfile.Key(1, str))


def save_params(path: str, p: ObstacleParams) -> None:
    """Floats as repr, so load_params(save_params(p)) == p exactly."""
    paramfile.write(path, "obstacle grid and laser scan: base_from_cam = row-major 3x4 [R|t] (all zero: level forward mount), metres, radians",
                    _FILE, [(k, getattr(p, k)) for k in ("base_from_cam",) + _FLOATS + _INTS + ("frame",)])


def load_params(path: str) -> ObstacleParams:
    """A key that is missing keeps ObstacleParams' default; an unknown or repeated key, or a wrong number of values, is an error."""
    return ObstacleParams(**paramfile.read(path, _FILE))


# ---- what `filelist --obstacles` writes ------------------------------------------------------------------------------------------
def grid_image(occ: np.ndarray) -> np.ndarray:
    """occ int8 (gh, gw) -> uint8 (gw, gh) picture with forward up and left to the left: 0 occupied, 128 unknown, 255 free."""
    o = np.asarray(occ, np.int8)
    g = np.where(o == OCCUPIED, 0, np.where(o == FREE, 255, 128)).astype(np.uint8)      # [iy][ix]
    return np.ascontiguousarray(g.T[::-1, ::-1])                                       # row = far x first, column = large y first


def write_pgm(path: str, img: np.ndarray) -> None:
    img = np.ascontiguousarray(img, np.uint8)
    with open(path, "wb") as f:
        f.write(f"P5\n{img.shape[1]} {img.shape[0]}\n255\n".encode("ascii"))
        f.write(img.tobytes())


def write_scan(path: str, p: ObstacleParams, ranges: np.ndarray) -> None:
    """one `angle range` line per beam: the beam's centre angle in radians, the range in metres (inf without a return)"""
    with open(path, "w") as f:
        for a, r in zip(beam_angles(p), np.asarray(ranges, np.float32).reshape(-1)):
            f.write(f"{a:.6f} {float(r)!r}\n")
