"""Rolling elevation map and step-height traversability: the parameters of ``sn_elevation`` (include/stereonet_hip.h), the Python
pose quantiser, a vectorised numpy twin of the update (bit-exact: everything below the pose quantisation is integer or a single
rounded fp32 operation) with its state carried in an object, a plain loop over Python integers written from the header against
which the twin is checked, the parameter file, and the pictures of the planes.

The samples are the point cloud's and the base frame is the obstacle stage's.  A "sub" is 1/256 of a cell; heights are
millimetres.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Tuple

import numpy as np

from . import obstacles, paramfile, pointcloud, spec, torus

MAX_WINDOW = 4096                   # mw, mh
UNKNOWN = -32768                    # hi and lo of a cell nobody has observed
Q30 = 1 << 30
_I32_MIN, _I32_MAX = -(1 << 31), (1 << 31) - 1
F32 = np.float32


@dataclasses.dataclass
class ElevationParams:
    """sn_elevation_params.  frame is the fixed frame's id for the node's publisher, feed_inflate (0 or 1) whether the node inflates
    this grid instead of the costmap's or the obstacle grid (neither is part of the struct)."""
    mw: int = 200
    mh: int = 200
    cell_m: float = 0.1
    base_from_cam: Tuple[float, ...] = (0.0,) * 12
    z_min_m: float = -1.0
    z_max_m: float = 1.5
    range_max_m: float = 6.0
    min_points: int = 3
    alpha: int = 128
    max_step_mm: int = 60
    radius: int = 1
    flags: int = 0
    frame: str = "odom"
    feed_inflate: int = 0

    def matrix(self) -> np.ndarray:
        """the twelve float32 the arithmetic uses"""
        m = np.asarray(self.base_from_cam, F32).reshape(12)
        return np.asarray(obstacles.LEVEL_MOUNT, F32) if not m.any() else m


_FLOATS = ("cell_m", "z_min_m", "z_max_m", "range_max_m")
_INTS = ("mw", "mh", "min_points", "alpha", "max_step_mm", "radius", "flags")


def check(p: ElevationParams) -> Optional[str]:
    """None, or why sn_elevation_create refuses these parameters."""
    if p.mw < 1 or p.mh < 1 or p.mw > MAX_WINDOW or p.mh > MAX_WINDOW:
        return "mw and mh must be 1..4096"
    if len(p.base_from_cam) != 12 or not np.all(np.isfinite(np.asarray(p.base_from_cam, F32))):
        return "base_from_cam must be twelve finite numbers"
    vals = np.asarray([getattr(p, k) for k in _FLOATS], F32)
    if not np.all(np.isfinite(vals)):
        return "every parameter must be finite"
    if not F32(p.cell_m) > 0:
        return "cell_m must be positive"
    if F32(p.z_min_m) < -32 or F32(p.z_max_m) > 32 or F32(p.z_min_m) > F32(p.z_max_m):
        return "-32 <= z_min_m <= z_max_m <= 32 is required"
    if not F32(p.range_max_m) > 0:
        return "range_max_m must be positive"
    if p.min_points < 1:
        return "min_points must be at least 1"
    if not 1 <= p.alpha <= 256:
        return "alpha must be 1..256"
    if not 1 <= p.max_step_mm <= 32767:
        return "max_step_mm must be 1..32767"
    if not 1 <= p.radius <= 3:
        return "radius must be 1..3"
    if p.flags != 0:
        return "flags must be 0"
    return None


@dataclasses.dataclass(frozen=True)
class Units:
    """the host quantities of the contract"""
    k256: float
    k256f: np.float32
    zmin_mm: int
    zmax_mm: int


def units(p: ElevationParams) -> Units:
    k256 = 256.0 / float(F32(p.cell_m))
    return Units(k256, F32(k256), int(np.floor(F32(p.z_min_m) * F32(1000.0))), int(np.floor(F32(p.z_max_m) * F32(1000.0))))


def pose_q(p: ElevationParams, pose) -> np.ndarray:
    """sn_elevation_pose_q: (x, y, yaw) -> int32 (6,) = {tx, ty, cq, sq, ox, oy}.  ValueError for a pose that is not finite or
    too far.  The library's may differ by one unit in cq, sq: two implementations of a double cos and sin."""
    return torus.pose_q(units(p).k256, p.mw, p.mh, pose)


def base_points(raw: np.ndarray, cam: pointcloud.Camera, mounts: np.ndarray, out_scale: float = spec.OUT_SCALE):
    """raw int32 (n, H, W), mounts float32 (n, 12) -> (xb, yb, zb) float32 (n, Ho, Wo): the base-frame coordinates of every
    sample as the obstacle stage computes them, NaN where the sample is not valid."""
    pts, _ = pointcloud.reference(np.asarray(raw, np.int32), cam, pointcloud.ORGANISED, out_scale=out_scale)
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    m = np.asarray(mounts, F32).reshape(-1, 12)[:, :, None, None]
    with np.errstate(invalid="ignore", over="ignore"):
        return tuple(((m[:, 4 * i] * x + m[:, 4 * i + 1] * y) + m[:, 4 * i + 2] * z) + m[:, 4 * i + 3] for i in range(3))


def accumulate(p: ElevationParams, q, xb: np.ndarray, yb: np.ndarray, zb: np.ndarray):
    """step 2 of the contract for one frame: the base-frame samples (any shape) -> (cnt, fmax, fmin) int64 (mh, mw), unrolled"""
    u = units(p)
    tx, ty, cq, sq, ox, oy = (int(v) for v in q)
    xb, yb, zb = (np.asarray(a, F32).reshape(-1) for a in (xb, yb, zb))
    with np.errstate(invalid="ignore", over="ignore"):
        ok = ~np.isnan(zb)
        zf = np.floor(zb * F32(1000.0))
        zmm = np.clip(np.where(ok, zf, 0).astype(np.float64), _I32_MIN, _I32_MAX).astype(np.int64)
        ok &= (u.zmin_mm <= zmm) & (zmm <= u.zmax_mm)
        ok &= np.sqrt(xb * xb + yb * yb) <= F32(p.range_max_m)
        sxf, syf = np.floor(xb * u.k256f), np.floor(yb * u.k256f)
        ok &= (np.abs(sxf) < F32(Q30)) & (np.abs(syf) < F32(Q30))
    sx, sy, zmm = sxf[ok].astype(np.int64), syf[ok].astype(np.int64), zmm[ok]
    wx = tx + ((cq * sx - sq * sy + (1 << 29)) >> 30)
    wy = ty + ((sq * sx + cq * sy + (1 << 29)) >> 30)
    cx, cy = (wx >> 8) - ox, (wy >> 8) - oy
    inside = (cx >= 0) & (cx < p.mw) & (cy >= 0) & (cy < p.mh)
    cell, zmm = (cy[inside] * p.mw + cx[inside]), zmm[inside]
    cells = p.mw * p.mh
    cnt = np.bincount(cell, minlength=cells).astype(np.int64)
    fmax, fmin = np.full(cells, _I32_MIN, np.int64), np.full(cells, _I32_MAX, np.int64)
    np.maximum.at(fmax, cell, zmm)
    np.minimum.at(fmin, cell, zmm)
    return cnt.reshape(p.mh, p.mw), fmax.reshape(p.mh, p.mw), fmin.reshape(p.mh, p.mw)


def verdict(p: ElevationParams, hi: np.ndarray, lo: np.ndarray):
    """step 4 on unrolled planes (mh, mw) -> (trav int8, rise uint16)"""
    hi, lo = np.asarray(hi, np.int64), np.asarray(lo, np.int64)
    known, r = hi != UNKNOWN, p.radius
    hp = np.pad(np.where(known, hi, UNKNOWN), r, constant_values=UNKNOWN)
    lp = np.pad(np.where(known, lo, 32767), r, constant_values=32767)
    mx, mn = np.full(hi.shape, UNKNOWN, np.int64), np.full(hi.shape, 32767, np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            mx = np.maximum(mx, hp[dy:dy + p.mh, dx:dx + p.mw])
            mn = np.minimum(mn, lp[dy:dy + p.mh, dx:dx + p.mw])
    rise = np.where(known, np.maximum(mx - lo, hi - mn), 0)
    trav = np.where(known, np.where(rise > p.max_step_mm, 100, 0), -1)
    return trav.astype(np.int8), np.minimum(rise, 65535).astype(np.uint16)


class Reference:
    """The header's arithmetic on the host, vectorised over the window: per stream the two int16 planes on the torus and the
    origin of the last frame."""

    def __init__(self, p: ElevationParams, streams: int = 1):
        why = check(p)
        if why:
            raise ValueError(why)
        self.p = p
        self.hi = np.full((streams, p.mh, p.mw), UNKNOWN, np.int16)
        self.lo = np.full((streams, p.mh, p.mw), UNKNOWN, np.int16)
        self.origin = [None] * streams
        self.frames = []      # per frame pushed: how many cells took each branch of the contract (what the tests' inputs are judged by)

    def reset(self, stream: int = -1):
        for s in (range(len(self.origin)) if stream < 0 else [stream]):
            self.hi[s], self.lo[s] = UNKNOWN, UNKNOWN
            self.origin[s] = None

    def push(self, q, raw, cam: pointcloud.Camera, mounts=None, stream_of=None, out_scale: float = spec.OUT_SCALE):
        """q int (n, 6) (the library's, or pose_q's), raw int32 (n, H, W), mounts float32 (n, 12) or None (the parameters'
        mount) -> (trav int8, hi int16, lo int16, rise uint16, each (n, mh, mw), stats uint32 (n, 4))"""
        p = self.p
        q = np.asarray(q, np.int64).reshape(-1, 6)
        n = q.shape[0]
        raw = np.asarray(raw, np.int32).reshape((n,) + np.shape(raw)[-2:])
        m = np.tile(p.matrix(), (n, 1)) if mounts is None else np.asarray(mounts, F32).reshape(n, 12)
        xb, yb, zb = base_points(raw, cam, m, out_scale)
        ids = np.zeros(n, np.int64) if stream_of is None else np.asarray(stream_of, np.int64).reshape(n)
        trav, rise = np.empty((n, p.mh, p.mw), np.int8), np.empty((n, p.mh, p.mw), np.uint16)
        hi, lo = np.empty((n, p.mh, p.mw), np.int16), np.empty((n, p.mh, p.mw), np.int16)
        stats = np.zeros((n, 4), np.uint32)
        for k in range(n):
            trav[k], hi[k], lo[k], rise[k], stats[k] = self.frame(int(ids[k]), q[k], accumulate(p, q[k], xb[k], yb[k], zb[k]))
        return trav, hi, lo, rise, stats

    def frame(self, s: int, q, acc):
        """steps 1, 3 and 4 for the accumulators `acc` = (cnt, fmax, fmin) of one frame of stream s"""
        p = self.p
        cnt, fmax, fmin = acc
        ox, oy = int(q[4]), int(q[5])
        br = dict(stream=s, scrolled=0, born=0, blended=0, clamped=0, up=0, down=0, prev=self.origin[s], origin=(ox, oy))
        self.frames.append(br)
        _, _, moved, rows, cols = torus.view(p.mw, p.mh, (ox, oy), self.origin[s])
        H, L = self.hi[s].astype(np.int64), self.lo[s].astype(np.int64)
        if moved is not None:
            br["scrolled"] = int((moved & (H != UNKNOWN)).sum())
            H[moved], L[moved] = UNKNOWN, UNKNOWN
        c, fx, fn = cnt[rows, cols], fmax[rows, cols], fmin[rows, cols]
        fused, known = c >= p.min_points, H != UNKNOWN
        clamp = lambda v: np.clip(v, -32767, 32767)      # noqa: E731
        bh = H + (((fx - H) * p.alpha + 128) >> 8)
        bl = L + (((fn - L) * p.alpha + 128) >> 8)
        nh = np.where(fused, np.where(known, clamp(bh), clamp(fx)), H)
        nl = np.where(fused, np.where(known, clamp(bl), clamp(fn)), L)
        br["born"], br["blended"] = int((fused & ~known).sum()), int((fused & known).sum())
        br["up"], br["down"] = int((fused & known & (nh > H)).sum()), int((fused & known & (nh < H)).sum())
        br["clamped"] = int((fused & ((np.where(known, bh, fx) != nh) | (np.where(known, bl, fn) != nl))).sum())
        self.hi[s], self.lo[s] = nh.astype(np.int16), nl.astype(np.int16)
        self.origin[s] = (ox, oy)
        hi, lo = np.empty(H.shape, np.int16), np.empty(H.shape, np.int16)
        hi[rows, cols], lo[rows, cols] = nh, nl
        trav, rise = verdict(p, hi, lo)
        return trav, hi, lo, rise, np.array([(hi != UNKNOWN).sum(), (trav == 100).sum(), fused.sum(), cnt.sum()], np.uint32)


def reference(p: ElevationParams, q, raw, cam, mounts=None, stream_of=None, streams: int = 1):
    """one push of a fresh Reference"""
    return Reference(p, streams).push(q, raw, cam, mounts, stream_of)


class LoopReference:
    """The header again, sample by sample and cell by cell over Python integers (the fp32 steps on numpy float32 scalars): what
    Reference is checked against (slow: small maps and windows only)."""

    def __init__(self, p: ElevationParams, streams: int = 1):
        self.p, self.u = p, units(p)
        self.hi = [[[UNKNOWN] * p.mw for _ in range(p.mh)] for _ in range(streams)]
        self.lo = [[[UNKNOWN] * p.mw for _ in range(p.mh)] for _ in range(streams)]
        self.origin = [None] * streams

    def reset(self, stream: int = -1):
        p = self.p
        for s in (range(len(self.origin)) if stream < 0 else [stream]):
            self.hi[s] = [[UNKNOWN] * p.mw for _ in range(p.mh)]
            self.lo[s] = [[UNKNOWN] * p.mw for _ in range(p.mh)]
            self.origin[s] = None

    def accumulate(self, q, xb, yb, zb):
        p, u = self.p, self.u
        tx, ty, cq, sq, ox, oy = (int(v) for v in q)
        cnt = [[0] * p.mw for _ in range(p.mh)]
        fmax = [[_I32_MIN] * p.mw for _ in range(p.mh)]
        fmin = [[_I32_MAX] * p.mw for _ in range(p.mh)]
        with np.errstate(invalid="ignore", over="ignore"):
            for x, y, z in zip(np.asarray(xb, F32).reshape(-1), np.asarray(yb, F32).reshape(-1), np.asarray(zb, F32).reshape(-1)):
                if z != z:
                    continue
                zf = float(np.floor(z * F32(1000.0)))
                zmm = _I32_MAX if zf >= 2.0 ** 31 else _I32_MIN if zf <= -2.0 ** 31 else int(zf)
                if not u.zmin_mm <= zmm <= u.zmax_mm:
                    continue
                xx, yy = x * x, y * y
                if not np.sqrt(xx + yy) <= F32(p.range_max_m):
                    continue
                sxf, syf = float(np.floor(x * u.k256f)), float(np.floor(y * u.k256f))
                if not (abs(sxf) < Q30 and abs(syf) < Q30):
                    continue
                sx, sy = int(sxf), int(syf)
                wx = tx + ((cq * sx - sq * sy + (1 << 29)) >> 30)
                wy = ty + ((sq * sx + cq * sy + (1 << 29)) >> 30)
                cx, cy = (wx >> 8) - ox, (wy >> 8) - oy
                if 0 <= cx < p.mw and 0 <= cy < p.mh:
                    cnt[cy][cx] += 1
                    fmax[cy][cx], fmin[cy][cx] = max(fmax[cy][cx], zmm), min(fmin[cy][cx], zmm)
        return cnt, fmax, fmin

    def push(self, q, raw, cam: pointcloud.Camera, mounts=None, stream_of=None, out_scale: float = spec.OUT_SCALE):
        p = self.p
        q = [[int(v) for v in row] for row in np.asarray(q).reshape(-1, 6)]
        n = len(q)
        raw = np.asarray(raw, np.int32).reshape((n,) + np.shape(raw)[-2:])
        m = np.tile(p.matrix(), (n, 1)) if mounts is None else np.asarray(mounts, F32).reshape(n, 12)
        xb, yb, zb = base_points(raw, cam, m, out_scale)
        trav, rise = np.empty((n, p.mh, p.mw), np.int8), np.empty((n, p.mh, p.mw), np.uint16)
        hi, lo = np.empty((n, p.mh, p.mw), np.int16), np.empty((n, p.mh, p.mw), np.int16)
        stats = np.zeros((n, 4), np.uint32)
        clamp = lambda v: min(max(v, -32767), 32767)      # noqa: E731
        for k in range(n):
            s = 0 if stream_of is None else int(stream_of[k])
            ox, oy = q[k][4], q[k][5]
            cnt, fmax, fmin = self.accumulate(q[k], xb[k], yb[k], zb[k])
            Hs, Ls, prev = self.hi[s], self.lo[s], self.origin[s]
            known = fused = points = 0
            for j in range(p.mh):
                for i in range(p.mw):
                    cx, cy = ox + (i - ox) % p.mw, oy + (j - oy) % p.mh
                    h, l = Hs[j][i], Ls[j][i]
                    if prev is not None and (cx != prev[0] + (i - prev[0]) % p.mw or cy != prev[1] + (j - prev[1]) % p.mh):
                        h = l = UNKNOWN
                    c = cnt[cy - oy][cx - ox]
                    points += c
                    if c >= p.min_points:
                        fx, fn = fmax[cy - oy][cx - ox], fmin[cy - oy][cx - ox]
                        if h == UNKNOWN:
                            h, l = clamp(fx), clamp(fn)
                        else:
                            h = clamp(h + (((fx - h) * p.alpha + 128) >> 8))
                            l = clamp(l + (((fn - l) * p.alpha + 128) >> 8))
                        fused += 1
                    Hs[j][i], Ls[j][i] = h, l
                    known += h != UNKNOWN
                    hi[k, cy - oy, cx - ox], lo[k, cy - oy, cx - ox] = h, l
            self.origin[s] = (ox, oy)
            lethal = 0
            for y in range(p.mh):
                for x in range(p.mw):
                    hc, lc = int(hi[k, y, x]), int(lo[k, y, x])
                    if hc == UNKNOWN:
                        trav[k, y, x], rise[k, y, x] = -1, 0
                        continue
                    r = 0
                    for yy in range(max(y - p.radius, 0), min(y + p.radius, p.mh - 1) + 1):
                        for xx in range(max(x - p.radius, 0), min(x + p.radius, p.mw - 1) + 1):
                            if int(hi[k, yy, xx]) != UNKNOWN:
                                r = max(r, int(hi[k, yy, xx]) - lc, hc - int(lo[k, yy, xx]))
                    trav[k, y, x], rise[k, y, x] = (100 if r > p.max_step_mm else 0), min(r, 65535)
                    lethal += r > p.max_step_mm
            stats[k] = (known, lethal, fused, points)
        return trav, hi, lo, rise, stats


# ---- synthetic clips for the tests and the benchmark -----------------------------------------------------------------------------
def terrain_map(w: int, h: int, cam: pointcloud.Camera, cam_height_m: float, wall_z_m: float, seed: int = 0, rough_m: float = 0.05,
                holes: float = 0.1, out_scale: float = spec.OUT_SCALE) -> np.ndarray:
    """A synthetic map, int32 (h, w): obstacles.ground_and_wall with the ground's height disturbed per pixel by up to rough_m
    (so cells get a spread between hi and lo, and steps between neighbours), and a share `holes` of the pixels without a
    disparity (0) or with a negative one."""
    rng = np.random.default_rng(seed)
    c = cam.resolved(w, h)
    dv = np.arange(h, dtype=np.float64)[:, None] - c.cy
    height = cam_height_m + rng.uniform(-rough_m, rough_m, (h, w))
    zg = np.where(dv > 0, height * c.fy / np.where(dv > 0, dv, 1.0), np.inf)
    z = np.minimum(zg, wall_z_m)
    raw = np.rint(c.fx * c.baseline_mm / (z * 1000.0 * 16.0 * 12.0 * out_scale)).astype(np.int32)
    bad = rng.random((h, w)) < holes
    raw[bad] = rng.choice(np.array([0, -5], np.int32), int(bad.sum()))
    return raw


def synthetic_clip(p: ElevationParams, w: int, h: int, cam: pointcloud.Camera, n: int, seed: int = 0, step_cells: float = 2.5, rough_m: float = 0.01):
    """-> (poses float64 (n, 3), raw int32 (n, h, w)): a random walk whose steps scroll the window by a cell or two, in front of
    rough ground whose height rises and falls by a few centimetres from frame to frame and a wall whose distance changes"""
    rng = np.random.default_rng(seed)
    step = step_cells * float(p.cell_m)
    poses = np.cumsum(rng.normal(0.0, 1.0, (n, 3)) * (step, step, 0.3), axis=0) + (-1.0, 0.5, 0.0)
    raw = np.stack([terrain_map(w, h, cam, 0.4 + 0.06 * ((2 * k) % 3), 1.5 + 0.5 * (k % 4), seed * 100 + k, rough_m) for k in range(n)])
    return poses, raw


# ---- the parameter file: one `key value` per line, `#` comments, as obstacles.py's ------------------------------------------------
_FILE = paramfile.spec(_FLOATS, _INTS + ("feed_inflate",), base_from_cam=paramfile.Key(12), frame=paramfile.Key(1, str))


def save_params(path: str, p: ElevationParams) -> None:
    """Floats as repr, so load_params(save_params(p)) == p exactly."""
    paramfile.write(path, "rolling elevation map: window in cells of cell_m, heights in metres and millimetres, base_from_cam row-major 3x4",
                    _FILE, [(k, getattr(p, k)) for k in _INTS + _FLOATS + ("base_from_cam", "frame", "feed_inflate")])


def load_params(path: str) -> ElevationParams:
    """A key that is missing keeps ElevationParams' default; an unknown or repeated key, or a wrong number of values, is an
    error."""
    got = paramfile.read(path, _FILE)
    if got.get("feed_inflate", 0) not in (0, 1):
        raise ValueError(f"{path}: feed_inflate must be 0 or 1")
    return ElevationParams(**got)


# ---- pictures of the planes ---------------------------------------------------------------------------------------------------
def trav_image(trav: np.ndarray) -> np.ndarray:
    """trav int8 (mh, mw) -> uint8 (mw, mh) picture with world x up and y to the left: 255 drivable, 0 lethal, 128 unknown"""
    t = np.asarray(trav, np.int16)
    img = np.where(t < 0, 128, np.where(t >= 100, 0, 255)).astype(np.uint8)
    return np.ascontiguousarray(img.T[::-1, ::-1])


def height_image(hi: np.ndarray, lo_mm: int = -1000, hi_mm: int = 1000) -> np.ndarray:
    """hi int16 (mh, mw) -> uint8 (mw, mh) picture, oriented as trav_image: 1..255 from lo_mm to hi_mm, 0 unknown"""
    v = np.asarray(hi, np.int64)
    g = 1 + (np.clip(v, lo_mm, hi_mm) - lo_mm) * 254 // max(hi_mm - lo_mm, 1)
    return np.ascontiguousarray(np.where(v == UNKNOWN, 0, g).astype(np.uint8).T[::-1, ::-1])
