"""Inflation of occupancy grids by the robot's radius: the parameters of ``sn_inflate_grid`` (include/stereonet_hip.h), the
refusals of the C side in its words, the Python restatement of the host cost table, a vectorised numpy twin (bit-exact when it is
fed the library's table: everything below the table is integer), a plain brute-force loop over Python integers written from the
header against which the twin is checked, the publisher's translation of a cost, the parameter file of the tools and the node,
and one small batch that takes every branch of the contract.

The input is an OccupancyGrid payload as the obstacle stage (``occ``) and the costmap (``grid``) write it: -1 unknown, 0..100
known.  ``d2`` is a squared distance in cells.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import numpy as np

from . import paramfile

MAX_R = 64                          # SN_INFLATE_MAX_R
MAX_CELLS = 4096                    # gw, gh
UNKNOWN = 1                         # SN_INFLATE_UNKNOWN
NOT_REACHED = 0xFFFF                # dist2 of a cell further than R from every obstacle
STATS = ("lethal", "inscribed", "inflated", "free", "unknown")      # stats[k]: cells at 254, 253, 1..252, 0, 255
BRANCHES = ("obstacle", "inscribed", "decayed", "at_r2", "past_r2", "decayed_to_zero", "unknown_kept", "unknown_lethal",
            "unknown_flag_only", "below_lethal_min", "at_lethal_min")


@dataclasses.dataclass
class InflateParams:
    """sn_inflate_params.  The tools and the node take cell_m from the grid they inflate; frame-less: the output has its source's."""
    cell_m: float = 0.05
    inscribed_radius_m: float = 0.2
    inflation_radius_m: float = 0.4
    cost_scaling: float = 10.0
    lethal_min: int = 100
    flags: int = 0


_FLOATS = ("cell_m", "inscribed_radius_m", "inflation_radius_m", "cost_scaling")
_INTS = ("lethal_min", "flags")


def _f(v) -> float:
    """the struct holds fp32"""
    with np.errstate(over="ignore"):
        return float(np.float32(v))


def radius_cells(p: InflateParams) -> int:
    """R of the contract (for parameters check accepts)"""
    return int(math.ceil(_f(p.inflation_radius_m) / _f(p.cell_m)))


def check(p: InflateParams) -> Optional[str]:
    """None, or why sn_inflate_table refuses these parameters (a table that increases apart: table says)."""
    cell, ins, infl, k = (_f(getattr(p, name)) for name in _FLOATS)
    if not math.isfinite(cell) or not cell > 0:
        return "cell_m must be finite and positive"
    if not math.isfinite(ins) or ins < 0:
        return "inscribed_radius_m must be finite and not negative"
    if not math.isfinite(infl) or infl < ins:
        return "inflation_radius_m must be finite and at least inscribed_radius_m"
    if not math.isfinite(k) or k < 0:
        return "cost_scaling must be finite and not negative"
    if not math.ceil(infl / cell) <= MAX_R:
        return "the inflation radius must be at most 64 cells"
    if not 1 <= p.lethal_min <= 100:
        return "lethal_min must be 1..100"
    if p.flags & ~UNKNOWN:
        return "flags has bits other than SN_INFLATE_UNKNOWN"
    return None


def table(p: InflateParams) -> np.ndarray:
    """The header's table in Python doubles -> uint8 (R*R + 1,).  The library's may differ by ONE in an entry of the fall-off:
    two implementations of a double exp may differ by an ulp, and the product is truncated.  So reference() is fed the library's
    table (api.inflate_table), as the other twins are fed the beam table and the costmap's q."""
    why = check(p)
    if why:
        raise ValueError(why)
    cell, ins, infl, k = (_f(getattr(p, name)) for name in _FLOATS)
    R = radius_cells(p)
    T = np.zeros(R * R + 1, np.uint8)
    T[0] = 254
    for d2 in range(1, R * R + 1):
        dist = math.sqrt(float(d2)) * cell
        T[d2] = 253 if dist <= ins else 0 if dist > infl else int(252.0 * math.exp(-k * (dist - ins)))
    if np.any(np.diff(T.astype(np.int16)) > 0):
        raise ValueError("the cost table increases with the distance")
    return T


def translate(cost: np.ndarray) -> np.ndarray:
    """cost uint8 -> int8, the publisher's translation: 0 -> 0, 253 -> 99, 254 -> 100, 255 -> -1, else 1 + 97 * (c - 1) / 251"""
    c = np.asarray(cost, np.uint8).astype(np.int32)
    mid = 1 + 97 * (c - 1) // 251
    return np.where(c == 0, 0, np.where(c == 255, -1, np.where(c == 254, 100, np.where(c == 253, 99, mid)))).astype(np.int8)


def _within(p: InflateParams, R: int) -> np.ndarray:
    """bool (R*R + 1,): sqrt(d2) * cell_m <= inflation_radius_m, in the table's arithmetic"""
    cell, infl = _f(p.cell_m), _f(p.inflation_radius_m)
    return np.array([math.sqrt(float(d2)) * cell <= infl for d2 in range(R * R + 1)], bool)


def _finish(occ, d2, p, T, R):
    """(occ int (n, gh, gw), d2 int (n, gh, gw): exact wherever <= (R + 1)^2, larger elsewhere) -> the outputs and the branches"""
    reached = d2 <= R * R
    c = np.where(reached, T[np.minimum(d2, R * R)], 0).astype(np.int32)
    known = occ >= 0
    take = known | ((c > 0) if p.flags & UNKNOWN else (c >= 253))
    cost = np.where(take, c, 255).astype(np.uint8)
    dist2 = np.where(reached, d2, NOT_REACHED).astype(np.uint16)
    stats = np.stack([(cost == 254).sum((1, 2)), (cost == 253).sum((1, 2)), ((cost >= 1) & (cost <= 252)).sum((1, 2)),
                      (cost == 0).sum((1, 2)), (cost == 255).sum((1, 2))], 1).astype(np.uint32)
    inside = reached & _within(p, R)[np.minimum(d2, R * R)]
    br = dict(obstacle=d2 == 0, inscribed=reached & (c == 253), decayed=reached & (c >= 1) & (c <= 252), at_r2=(d2 == R * R) & (d2 > 0),
              past_r2=d2 == R * R + 1, decayed_to_zero=inside & (d2 > 0) & (c == 0), unknown_kept=~known & (c == 0),
              unknown_lethal=~known & (c >= 253), unknown_flag_only=~known & (c > 0) & (c < 253),
              below_lethal_min=occ == p.lethal_min - 1, at_lethal_min=occ == p.lethal_min)
    return cost, translate(cost), dist2, stats, {k: int(v.sum()) for k, v in br.items()}


def _prepare(occ, p, table_):
    why = check(p)
    if why:
        raise ValueError(why)
    o = np.asarray(occ, np.int8)
    o = (o[None] if o.ndim == 2 else o).astype(np.int32)
    if o.ndim != 3 or o.shape[1] < 1 or o.shape[2] < 1 or o.shape[1] > MAX_CELLS or o.shape[2] > MAX_CELLS:
        raise ValueError("gw and gh must be 1..4096")
    R = radius_cells(p)
    T = table(p) if table_ is None else np.asarray(table_, np.uint8).reshape(R * R + 1)
    return o, R, T


def reference(occ, p: InflateParams, table=None):
    """occ int8 (gh, gw) or (n, gh, gw), table: the library's (None: this module's, which may differ by one) ->
    (cost uint8, grid int8, dist2 uint16 (each (n, gh, gw)), stats uint32 (n, 5), branches: how many cells took each branch of
    the contract, by BRANCHES).  Two separable passes, exact: the nearest obstacle of every row within R + 1 columns, then the
    minimum of hx^2 + dy^2 over the rows within R + 1."""
    table_ = table
    o, R, T = _prepare(occ, p, table_)
    n, gh, gw = o.shape
    S, BIG = R + 1, 1 << 20
    ob = o >= p.lethal_min
    hx = np.full((n, gh, gw), BIG, np.int64)
    for d in range(min(S, gw - 1), -1, -1):      # descending: the smallest distance is written last
        hx[:, :, d:][ob[:, :, :gw - d]] = d
        hx[:, :, :gw - d][ob[:, :, d:]] = d
    h2 = np.where(hx < BIG, hx * hx, BIG)
    d2 = h2.copy()
    for dy in range(1, min(S, gh - 1) + 1):
        d2[:, dy:] = np.minimum(d2[:, dy:], h2[:, :gh - dy] + dy * dy)
        d2[:, :gh - dy] = np.minimum(d2[:, :gh - dy], h2[:, dy:] + dy * dy)
    return _finish(o, d2, p, T, R)


def loop_reference(occ, p: InflateParams, table=None):
    """The header again, cell by cell over Python integers and every obstacle of the map, the cost rule, the translation, dist2,
    the totals and the branch counts included: nothing is shared with reference but the table (slow: small grids only).  The
    same five results."""
    table_ = table
    o, R, T = _prepare(occ, p, table_)
    n, gh, gw = o.shape
    Tl, R2 = [int(v) for v in T], R * R
    cell, infl = _f(p.cell_m), _f(p.inflation_radius_m)
    cost, grid = np.empty((n, gh, gw), np.uint8), np.empty((n, gh, gw), np.int8)
    dist2, stats = np.empty((n, gh, gw), np.uint16), np.zeros((n, 5), np.uint32)
    br = dict.fromkeys(BRANCHES, 0)
    for k in range(n):
        rows = [[int(v) for v in row] for row in o[k]]
        obstacles = [(x, y) for y in range(gh) for x in range(gw) if rows[y][x] >= p.lethal_min]
        for y in range(gh):
            for x in range(gw):
                v = rows[y][x]
                d2 = min(((x - xo) * (x - xo) + (y - yo) * (y - yo) for (xo, yo) in obstacles), default=None)
                c = Tl[d2] if d2 is not None and d2 <= R2 else 0
                if v >= 0:
                    cst = c
                elif (c > 0) if p.flags & UNKNOWN else (c >= 253):
                    cst = c
                else:
                    cst = 255
                if cst == 0:
                    g = 0
                elif cst == 253:
                    g = 99
                elif cst == 254:
                    g = 100
                elif cst == 255:
                    g = -1
                else:
                    g = 1 + 97 * (cst - 1) // 251
                cost[k, y, x], grid[k, y, x] = cst, g
                dist2[k, y, x] = d2 if d2 is not None and d2 <= R2 else NOT_REACHED
                stats[k, 0 if cst == 254 else 1 if cst == 253 else 3 if cst == 0 else 4 if cst == 255 else 2] += 1
                reached = d2 is not None and d2 <= R2
                br["obstacle"] += d2 == 0
                br["inscribed"] += reached and c == 253
                br["decayed"] += reached and 1 <= c <= 252
                br["at_r2"] += d2 == R2 and d2 > 0
                br["past_r2"] += d2 == R2 + 1
                br["decayed_to_zero"] += reached and d2 > 0 and c == 0 and math.sqrt(float(d2)) * cell <= infl
                br["unknown_kept"] += v < 0 and c == 0
                br["unknown_lethal"] += v < 0 and c >= 253
                br["unknown_flag_only"] += v < 0 and 0 < c < 253
                br["below_lethal_min"] += v == p.lethal_min - 1
                br["at_lethal_min"] += v == p.lethal_min
    return cost, grid, dist2, stats, {k: int(v) for k, v in br.items()}


# ---- one batch that takes every branch ---------------------------------------------------------------------------------------------
BOUNDARY_P = InflateParams(cell_m=0.25, inscribed_radius_m=0.3, inflation_radius_m=1.0, cost_scaling=8.0, lethal_min=65, flags=0)


def boundary_scene():
    """-> (InflateParams, occ int8 (3, 21, 37)): R = 4 with d2 = 1 inscribed, d2 = 2..15 decayed and T[16] truncated to 0 inside
    the radius (252 * exp(-8 * 0.7) = 0.93).  Map 0: one obstacle at (18, 10), the columns left of it known and free, its own
    and those right of it unknown: inscribed, decayed and zeroed cells of both kinds, cells at d2 = 16 and 17, far cells.  Map 1:
    a random grid of unknown, free, values just below and at lethal_min, and 100.  Map 2: no obstacle at all (the skip path)."""
    rng = np.random.default_rng(19)
    occ = np.empty((3, 21, 37), np.int8)
    occ[0, :, :18], occ[0, :, 18:] = 0, -1
    occ[0, 10, 18] = 100
    occ[1] = rng.choice(np.array([-1, 0, 30, 64, 65, 100], np.int8), (21, 37), p=(0.4, 0.4, 0.1, 0.07, 0.015, 0.015))
    occ[2] = rng.choice(np.array([-1, 0, 64], np.int8), (21, 37), p=(0.5, 0.4, 0.1))
    return BOUNDARY_P, occ


# ---- the parameter file: one `key value` per line, `#` comments, as costmap.py's ---------------------------------------------------
_FILE = paramfile.spec(_FLOATS, _INTS)


def save_params(path: str, p: InflateParams) -> None:
    """Floats as repr, so load_params(save_params(p)) == p exactly."""
    paramfile.write(path, "inflation by the robot's radius: metres; flags 1 = an unknown cell takes any cost > 0; the tools and the node\n"
                    "# take cell_m from the grid they inflate", _FILE, [(k, getattr(p, k)) for k in _FLOATS + _INTS])


def load_params(path: str) -> InflateParams:
    """A key that is missing keeps InflateParams' default; an unknown or repeated key, or a wrong number of values, is an error."""
    return InflateParams(**paramfile.read(path, _FILE))


# ---- what `filelist --inflate` writes ---------------------------------------------------------------------------------------------
def write_pgm(path: str, cost: np.ndarray) -> None:
    """cost uint8 (gh, gw) -> a binary PGM of the cost bytes, row y of the grid as row y of the picture"""
    c = np.ascontiguousarray(cost, np.uint8)
    with open(path, "wb") as f:
        f.write(f"P5\n{c.shape[1]} {c.shape[0]}\n255\n".encode() + c.tobytes())
