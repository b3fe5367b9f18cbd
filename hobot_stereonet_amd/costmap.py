"""Rolling log-odds costmap with ray clearing: the parameters of ``sn_costmap`` (include/stereonet_hip.h), the Python pose
quantiser, a vectorised numpy twin of the update (bit-exact: everything below the pose quantisation is integer apart from two
single rounded double multiplies) with its state carried in an object, a plain loop over Python integers written from the
header against which the twin is checked, the parameter file of the tools and the node, and the picture ``filelist --costmap``
writes.

The inputs are the obstacle stage's: ``occ`` in the base-frame grid of an ``obstacles.ObstacleParams`` and ``ranges`` over its
beams.  A "sub" is 1/256 of a cell.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import numpy as np

from . import obstacles, paramfile, torus
from .obstacles import ObstacleParams

MAX_WINDOW = 4096                   # mw, mh
UNKNOWN_L = -32768                  # the state of a cell nobody has observed
_FAR, _CAP = 1 << 40, 1 << 31       # where gx0 / gy0 and margin / rmin / cmax saturate


@dataclasses.dataclass
class CostmapParams:
    """sn_costmap_params.  frame is the node's frame id (not part of the struct)."""
    mw: int = 200
    mh: int = 200
    l_hit: int = 85
    l_miss: int = 40
    l_min: int = -200
    l_max: int = 350
    clear_margin_m: float = 0.1
    clear_min_m: float = 0.0
    clear_max_m: float = 0.0
    frame: str = "odom"


_FLOATS = ("clear_margin_m", "clear_min_m", "clear_max_m")
_INTS = ("mw", "mh", "l_hit", "l_miss", "l_min", "l_max")


def check(p: CostmapParams, op: ObstacleParams) -> Optional[str]:
    """None, or why sn_costmap_create refuses these parameters (the sector of a scan apart: obstacles.beam_edges says)."""
    if p.mw < 1 or p.mh < 1 or p.mw > MAX_WINDOW or p.mh > MAX_WINDOW:
        return "mw and mh must be 1..4096"
    if not (1 <= p.l_hit <= 32767 and 1 <= p.l_miss <= 32767):
        return "l_hit and l_miss must be 1..32767"
    if not (-32767 <= p.l_min < 0 < p.l_max <= 32767):
        return "-32767 <= l_min < 0 < l_max <= 32767 is required"
    vals = np.asarray([getattr(p, k) for k in _FLOATS] + [op.cell_m, op.x_min_m, op.y_min_m], np.float32)
    if not np.all(np.isfinite(vals)):
        return "every parameter must be finite"
    if np.any(vals[:3] < 0):
        return "the clear_* distances must not be negative"
    if not np.float32(op.cell_m) > 0:
        return "cell_m must be positive"
    if op.gw < 0 or op.gh < 0 or op.gw > obstacles.MAX_CELLS or op.gh > obstacles.MAX_CELLS or (op.gw == 0) != (op.gh == 0):
        return "gw and gh must be 1..4096, or both 0"
    if op.beams < 0 or op.beams > obstacles.MAX_BEAMS:
        return "beams must be 0..4096"
    if op.gw == 0 and op.beams == 0:
        return "neither a grid nor a scan"
    return None


def _rint(v: float, lim: int) -> int:
    """llrint of a finite double (ties to even), values beyond +-lim taken as +-lim"""
    return lim if v >= lim else -lim if v <= -lim else int(np.rint(v))


@dataclasses.dataclass(frozen=True)
class Units:
    """the host quantities of the contract"""
    k256: float
    gx0: int
    gy0: int
    margin: int
    rmin: int
    cmax: int


def units(p: CostmapParams, op: ObstacleParams) -> Units:
    f = lambda v: float(np.float32(v))      # noqa: E731  the struct holds fp32
    k256 = 256.0 / f(op.cell_m)
    return Units(k256, _rint(f(op.x_min_m) / f(op.cell_m) * 256.0, _FAR), _rint(f(op.y_min_m) / f(op.cell_m) * 256.0, _FAR),
                 _rint(f(p.clear_margin_m) * k256, _CAP), _rint(f(p.clear_min_m) * k256, _CAP), _rint(f(p.clear_max_m) * k256, _CAP))


def pose_q(p: CostmapParams, op: ObstacleParams, pose) -> np.ndarray:
    """sn_costmap_pose_q: (x, y, yaw) -> int32 (6,) = {tx, ty, cq, sq, ox, oy}.  ValueError for a pose that is not finite or too
    far.  The library's may differ by one unit in cq, sq: two implementations of a double cos and sin."""
    return torus.pose_q(units(p, op).k256, p.mw, p.mh, pose)


def return_subs(ranges: np.ndarray, k256: float) -> np.ndarray:
    """Rb: float32 (beams,) -> int64, the returns in subs, -1 without one"""
    r = np.asarray(ranges, np.float32)
    ok = np.isfinite(r) & (r > 0)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.floor(np.where(ok, r, 0).astype(np.float64) * k256)
    return np.where(ok, np.minimum(s, 2.0 ** 31 - 1).astype(np.int64), -1)


class Reference:
    """The header's arithmetic on the host, vectorised over the window: `streams` int16 maps and their origins."""

    def __init__(self, p: CostmapParams, op: ObstacleParams, streams: int = 1, edges: Optional[np.ndarray] = None):
        why = check(p, op)
        if why:
            raise ValueError(why)
        self.p, self.op, self.u = p, op, units(p, op)
        self.edges = None
        if op.beams:
            e = obstacles.beam_edges(op) if edges is None else np.asarray(edges, np.float32).reshape(op.beams + 1)
            self.edges = e.astype(np.float64)
        self.L = np.full((streams, p.mh, p.mw), UNKNOWN_L, np.int16)
        self.origin = [None] * streams
        self.frames = []      # per frame pushed: how many cells took each branch of the contract (what the tests' inputs are judged by)

    def reset(self, stream: int = -1):
        for s in (range(len(self.origin)) if stream < 0 else [stream]):
            self.L[s] = UNKNOWN_L
            self.origin[s] = None

    def push(self, q, occ=None, ranges=None, stream_of=None):
        """q int (n, 6) (the library's, or pose_q's), occ int8 (n, gh, gw) or None, ranges float32 (n, beams) or None ->
        (grid int8 (n, mh, mw), logodds int16 (n, mh, mw), stats uint32 (n, 4))"""
        p, op = self.p, self.op
        q = np.asarray(q, np.int64).reshape(-1, 6)
        n = q.shape[0]
        if op.gw == 0:
            occ = None
        if op.beams == 0:
            ranges = None
        if occ is None and ranges is None:
            raise ValueError("neither occ nor ranges")
        ids = np.zeros(n, np.int64) if stream_of is None else np.asarray(stream_of, np.int64).reshape(n)
        grid, logodds = np.empty((n, p.mh, p.mw), np.int8), np.empty((n, p.mh, p.mw), np.int16)
        stats = np.zeros((n, 4), np.uint32)
        for k in range(n):
            grid[k], logodds[k], stats[k] = self._frame(int(ids[k]), q[k], None if occ is None else np.asarray(occ, np.int8)[k],
                                                        None if ranges is None else np.asarray(ranges, np.float32)[k])
        return grid, logodds, stats

    def _frame(self, s, q, occ, ranges):
        p, op, u = self.p, self.op, self.u
        br = dict(stream=s, hit=0, clear_occ=0, clear_ray=0, ray_edge=0, ray_inside=0, at_min=0, at_max=0, born=0, scrolled=0,
                  prev=self.origin[s], origin=(int(q[4]), int(q[5])))
        self.frames.append(br)
        tx, ty, cq, sq, ox, oy = (int(v) for v in q)
        cx, cy, moved, rows, cols = torus.view(p.mw, p.mh, (ox, oy), self.origin[s])
        L = self.L[s].astype(np.int64)
        if moved is not None:
            br["scrolled"] = int((moved & (L != UNKNOWN_L)).sum())
            L[moved] = UNKNOWN_L
        dx, dy = (cx * 256 + 128 - tx)[None, :], (cy * 256 + 128 - ty)[:, None]
        bx = (cq * dx + sq * dy + (1 << 29)) >> 30
        by = (-sq * dx + cq * dy + (1 << 29)) >> 30
        o = np.full(L.shape, -1, np.int64)
        if occ is not None:
            qx, qy = (bx - u.gx0) >> 8, (by - u.gy0) >> 8
            inside = (qx >= 0) & (qx < op.gw) & (qy >= 0) & (qy < op.gh)
            o[inside] = occ.reshape(op.gh, op.gw)[qy[inside], qx[inside]]
        ray = np.zeros(L.shape, bool)
        if ranges is not None:
            E, fbx, fby = self.edges, bx.astype(np.float64), by.astype(np.float64)
            count = np.zeros(L.shape, np.int64)
            for e in E:
                count += e * fbx <= fby
            sector = (bx > 0) & (E[0] * fbx <= fby) & ~(E[-1] * fbx <= fby)
            Rb = return_subs(ranges, u.k256)[np.clip(count - 1, 0, op.beams - 1)]
            C, r2 = Rb - u.margin, bx * bx + by * by
            near = sector & (Rb >= 0) & (C > 0) & (r2 >= u.rmin * u.rmin) & ((r2 <= u.cmax * u.cmax) if u.cmax else True)
            ray = near & (r2 < C * C)
            br["ray_edge"] = int((near & (r2 == C * C)).sum())
            br["ray_inside"] = int((ray & (r2 >= (C - 1) * (C - 1))).sum())
        L0 = np.where(L == UNKNOWN_L, 0, L)
        hit = o == 100
        clear = ~hit & ((o == 0) | ray)
        new = np.where(hit, np.minimum(L0 + p.l_hit, p.l_max), np.where(clear, np.maximum(L0 - p.l_miss, p.l_min), L))
        br["hit"] = int(hit.sum())
        br["clear_occ"] = int((~hit & (o == 0)).sum())
        br["clear_ray"] = int((clear & (o != 0)).sum())
        br["at_min"] = int((clear & (new == p.l_min)).sum())
        br["at_max"] = int((hit & (new == p.l_max)).sum())
        br["born"] = int(((L == UNKNOWN_L) & (new != UNKNOWN_L)).sum())
        self.L[s] = new.astype(np.int16)
        self.origin[s] = (ox, oy)
        span = p.l_max - p.l_min
        known = new != UNKNOWN_L
        g = np.where(known, ((new - p.l_min) * 100 + span // 2) // span, -1)
        grid, logodds = np.empty(L.shape, np.int8), np.empty(L.shape, np.int16)
        grid[rows, cols] = g
        logodds[rows, cols] = new
        return grid, logodds, np.array([known.sum(), (known & (new > 0)).sum(), hit.sum(), clear.sum()], np.uint32)


def reference(p: CostmapParams, op: ObstacleParams, q, occ=None, ranges=None, stream_of=None, streams: int = 1, edges=None):
    """one push of a fresh Reference"""
    return Reference(p, op, streams, edges).push(q, occ, ranges, stream_of)


class LoopReference:
    """The header again, cell by cell over Python integers: what Reference is checked against (slow: small windows only)."""

    def __init__(self, p: CostmapParams, op: ObstacleParams, streams: int = 1, edges: Optional[np.ndarray] = None):
        self.p, self.op, self.u = p, op, units(p, op)
        e = (obstacles.beam_edges(op) if edges is None else edges) if op.beams else []
        self.E = [float(np.float32(v)) for v in e]
        self.L = [[[UNKNOWN_L] * p.mw for _ in range(p.mh)] for _ in range(streams)]
        self.origin = [None] * streams

    def reset(self, stream: int = -1):
        p = self.p
        for s in (range(len(self.origin)) if stream < 0 else [stream]):
            self.L[s] = [[UNKNOWN_L] * p.mw for _ in range(p.mh)]
            self.origin[s] = None

    def push(self, q, occ=None, ranges=None, stream_of=None):
        p, op, u = self.p, self.op, self.u
        q = [[int(v) for v in row] for row in np.asarray(q).reshape(-1, 6)]
        n = len(q)
        use_occ, use_rays = occ is not None and op.gw > 0, ranges is not None and op.beams > 0
        grid, logodds = np.empty((n, p.mh, p.mw), np.int8), np.empty((n, p.mh, p.mw), np.int16)
        stats = np.zeros((n, 4), np.uint32)
        span = p.l_max - p.l_min
        for k in range(n):
            s = 0 if stream_of is None else int(stream_of[k])
            tx, ty, cq, sq, ox, oy = q[k]
            Lmap, prev = self.L[s], self.origin[s]
            Rb = []
            if use_rays:
                for r in np.asarray(ranges, np.float32)[k]:
                    r = float(r)
                    Rb.append(min(math.floor(r * u.k256), 2 ** 31 - 1) if math.isfinite(r) and r > 0 else -1)
            known = pos = hits = cleared = 0
            for j in range(p.mh):
                for i in range(p.mw):
                    cx, cy = ox + (i - ox) % p.mw, oy + (j - oy) % p.mh
                    L = Lmap[j][i]
                    if prev is not None and (cx != prev[0] + (i - prev[0]) % p.mw or cy != prev[1] + (j - prev[1]) % p.mh):
                        L = UNKNOWN_L
                    dx, dy = cx * 256 + 128 - tx, cy * 256 + 128 - ty
                    bx = (cq * dx + sq * dy + (1 << 29)) >> 30
                    by = (-sq * dx + cq * dy + (1 << 29)) >> 30
                    o = -1
                    if use_occ:
                        qx, qy = (bx - u.gx0) >> 8, (by - u.gy0) >> 8
                        if 0 <= qx < op.gw and 0 <= qy < op.gh:
                            o = int(occ[k][qy][qx])
                    ray = False
                    if use_rays and bx > 0:
                        le = [e * float(bx) <= float(by) for e in self.E]
                        if le[0] and not le[-1]:
                            R = Rb[sum(le) - 1]
                            C, r2 = R - u.margin, bx * bx + by * by
                            ray = R >= 0 and C > 0 and r2 < C * C and r2 >= u.rmin * u.rmin and (u.cmax == 0 or r2 <= u.cmax * u.cmax)
                    L0 = 0 if L == UNKNOWN_L else L
                    if o == 100:
                        L = min(L0 + p.l_hit, p.l_max)
                        hits += 1
                    elif o == 0 or ray:
                        L = max(L0 - p.l_miss, p.l_min)
                        cleared += 1
                    Lmap[j][i] = L
                    known += L != UNKNOWN_L
                    pos += L > 0
                    grid[k, cy - oy, cx - ox] = -1 if L == UNKNOWN_L else ((L - p.l_min) * 100 + span // 2) // span
                    logodds[k, cy - oy, cx - ox] = L
            self.origin[s] = (ox, oy)
            stats[k] = (known, pos, hits, cleared)
        return grid, logodds, stats


# ---- synthetic clips for the tests and the benchmark -----------------------------------------------------------------------------
def synthetic_clip(p: CostmapParams, op: ObstacleParams, n: int, seed: int = 0, step_m: float = 0.3):
    """-> (poses float64 (n, 3), occ int8 (n, gh, gw), ranges float32 (n, beams)): a random walk whose steps scroll the window by
    a cell or two, grids of unknown / free / occupied cells, and returns inside the window with beams without one among them
    (inf, NaN, 0, negative)."""
    rng = np.random.default_rng(seed)
    poses = np.cumsum(rng.normal(0.0, 1.0, (n, 3)) * (step_m, step_m, 0.4), axis=0) + (-1.0, 0.5, 0.0)
    occ = rng.choice(np.array([-1, 0, 100], np.int8), (n, op.gh, op.gw), p=(0.5, 0.3, 0.2))
    reach = 0.5 * float(op.cell_m) * max(p.mw, p.mh)
    ranges = rng.uniform(0.1 * reach, 1.2 * reach, (n, op.beams)).astype(np.float32)
    if op.beams:
        bad = rng.random((n, op.beams)) < 0.2
        ranges[bad] = rng.choice(np.array([np.inf, np.nan, 0.0, -1.0, 1e30], np.float32), int(bad.sum()))
    return poses, occ, ranges


BOUNDARY_OP = ObstacleParams(x_min_m=0.0, y_min_m=-2.0, cell_m=0.25, gw=28, gh=16, beams=8, angle_min_rad=-0.8, angle_increment_rad=0.2,
                             range_min_m=0.0, range_max_m=20.0)
BOUNDARY_P = CostmapParams(mw=24, mh=18, l_hit=120, l_miss=70, l_min=-200, l_max=300, clear_margin_m=0.125, clear_min_m=0.3,
                           clear_max_m=2.5)


def boundary_clip():
    """-> (CostmapParams, ObstacleParams, poses (7, 3), occ (7, 16, 28), ranges (7, 8)): seven frames of one stream built so that
    every branch of the contract is taken.  Frames 0-2 stand at (0.125, 0.125) m with yaw 0, where a cell's base-frame centre is
    (cx*256, cy*256) subs: the centre of cell (4, 3) is at 1280 subs, exactly C of beam 7 (ranges 1.375 m less the margin of 128
    subs: not cleared), that of cell (5, 0) one sub inside C of beam 4; three equal grids drive cells to both clamps.  Frame 3
    scrolls back by one cell (yaw 0.3), which drops the column furthest ahead, frame 4 stands at negative y with yaw exactly pi/2, frame 5 scrolls the origin from -2 to 3
    (across the torus's wrap column) with yaw pi, frame 6 jumps further than a window."""
    p, op = BOUNDARY_P, BOUNDARY_OP
    rng = np.random.default_rng(18)
    poses = np.array([[0.125, 0.125, 0.0]] * 3 + [[-0.125, 0.125, 0.3], [2.6, -0.4, math.pi / 2], [3.9, -0.4, math.pi], [40.0, 25.0, -2.1]])
    occ = rng.choice(np.array([-1, 0, 100], np.int8), (7, op.gh, op.gw), p=(0.5, 0.3, 0.2))
    occ[1], occ[2] = occ[0], occ[0]
    occ[:3, 11, 4] = -1      # cell (4, 3) and cell (5, 0) are left to their rays
    occ[:3, 8, 5] = -1
    ranges = rng.uniform(0.5, 3.5, (7, op.beams)).astype(np.float32)
    ranges[:, 0], ranges[:, 1], ranges[:, 2], ranges[1, 3], ranges[2, 3] = np.inf, 0.0, np.nan, -1.0, 1e30
    ranges[:3, 7], ranges[:3, 4] = 1.375, 1409.0 / 1024.0
    return p, op, poses, occ, ranges


# ---- the parameter file: one `key value` per line, `#` comments, as obstacles.py's ------------------------------------------------
_FILE = paramfile.spec(_FLOATS, _INTS, frame=paramfile.Key(1, str))


def save_params(path: str, p: CostmapParams) -> None:
    """Floats as repr, so load_params(save_params(p)) == p exactly."""
    paramfile.write(path, "rolling log-odds costmap: window in cells of the obstacle grid's cell_m, log-odds in int16 units, metres",
                    _FILE, [(k, getattr(p, k)) for k in _INTS + _FLOATS + ("frame",)])


def load_params(path: str) -> CostmapParams:
    """A key that is missing keeps CostmapParams' default; an unknown or repeated key, or a wrong number of values, is an error."""
    return CostmapParams(**paramfile.read(path, _FILE))


def load_poses(path: str) -> np.ndarray:
    """one `x y yaw` line per frame (metres, radians; `#` comments) -> float64 (n, 3)"""
    rows = []
    with open(path) as f:
        for no, text in enumerate(f, 1):
            words = text.split("#", 1)[0].split()
            if not words:
                continue
            if len(words) != 3:
                raise ValueError(f"{path}:{no}: expected `x y yaw`")
            try:
                rows.append([float(v) for v in words])
            except ValueError:
                raise ValueError(f"{path}:{no}: not a number in {text.strip()!r}") from None
    return np.asarray(rows, np.float64).reshape(-1, 3)


# ---- what `filelist --costmap` writes -------------------------------------------------------------------------------------------
def grid_image(grid: np.ndarray) -> np.ndarray:
    """grid int8 (mh, mw), -1 or 0..100 -> uint8 (mw, mh) picture with world x up and y to the left, as obstacles.grid_image:
    255 free .. 0 occupied, 128 unknown."""
    g = np.asarray(grid, np.int16)
    img = np.where(g < 0, 128, 255 - (np.clip(g, 0, 100) * 255 + 50) // 100).astype(np.uint8)
    return np.ascontiguousarray(img.T[::-1, ::-1])


def write_pgm(path: str, grid: np.ndarray) -> None:
    obstacles.write_pgm(path, grid_image(grid))
