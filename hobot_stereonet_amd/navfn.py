"""The navigation function and the path to a goal over inflated cost grids: the parameters of ``sn_navfn``
(include/stereonet_hip.h), the refusals of the C side in its words, a numpy / heapq twin (Dijkstra from the goal: the field is the
unique fixed point of integer min-plus relaxation, so the twin and the kernel's tiled Bellman-Ford give the same words), a plain
relaxation loop over Python integers written from the header against which the twin is checked, the parameter file of the tools
and the node, and what ``filelist --plan`` writes.

The input is a cost grid as ``sn_inflate_grid`` writes it: 0 free, 1..252 graded, 253 inscribed, 254 lethal, 255 unknown.  Cells
are ``(x, y)``; north is ``y - 1``.
"""
from __future__ import annotations

import dataclasses
import heapq
from typing import Optional, Tuple

import numpy as np

from . import paramfile

TILE_W, TILE_H = 32, 32             # SN_NAV_TILE_W, SN_NAV_TILE_H: the tile of k_nav_relax
MAX_SIDE = 4096                     # gw, gh
MAX_AREA = 1 << 20                  # SN_NAV_MAX_CELLS: gw * gh
INF = 0xFFFFFFFF                    # SN_NAV_INF
UNKNOWN_OK = 1                      # SN_NAV_UNKNOWN_OK
GOAL_BLOCKED, START_UNREACHABLE, PATH_TRUNCATED, UNCONVERGED = 1, 2, 4, 8
STATS = ("flags", "reached", "path_cells", "p_start", "blocked")
# the eight neighbours in the order that breaks ties: E, NE, N, NW, W, SW, S, SE; odd = diagonal
MOVES = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))
MOVE_NAMES = ("E", "NE", "N", "NW", "W", "SW", "S", "SE")


@dataclasses.dataclass
class NavParams:
    """sn_nav_params, and for the tools the goal and the start in cells (the node takes them from SetGoal and the robot's pose)."""
    neutral: int = 50
    lethal_cost: int = 253
    unknown_cost: int = 0
    flags: int = 0
    max_rounds: int = 0
    max_path: int = 4096
    goal: Tuple[int, int] = (0, 0)
    start: Optional[Tuple[int, int]] = None


_INTS = ("neutral", "lethal_cost", "unknown_cost", "flags", "max_rounds", "max_path")
_CELLS = ("goal", "start")


def check(p: NavParams) -> Optional[str]:
    """None, or why sn_navfn refuses these parameters"""
    if not 1 <= p.neutral <= 255:
        return "neutral must be 1..255"
    if not 1 <= p.lethal_cost <= 255:
        return "lethal_cost must be 1..255"
    if not 0 <= p.unknown_cost <= 252:
        return "unknown_cost must be 0..252"
    if p.flags & ~UNKNOWN_OK:
        return "flags has bits other than SN_NAV_UNKNOWN_OK"
    if p.max_rounds < 0:
        return "max_rounds must not be negative"
    if p.max_path < 0:
        return "max_path must not be negative"
    return None


def weights(cost, p: NavParams) -> np.ndarray:
    """cost uint8 (...) -> int64 w of every cell, 0 where it is blocked; 255 is tested before lethal_cost"""
    c = np.asarray(cost, np.uint8).astype(np.int64)
    w = np.where(c >= p.lethal_cost, 0, p.neutral + c)
    return np.where(c == 255, (p.neutral + p.unknown_cost) if p.flags & UNKNOWN_OK else 0, w)


def worst_potential(cells: int) -> int:
    """the header's bound: a route leaves at most cells - 1 cells, each at no more than 7 * (255 + 254)"""
    return (cells - 1) * 7 * (255 + 254)


def _prepare(cost, goals, starts, p):
    why = check(p)
    if why:
        raise ValueError(why)
    c = np.asarray(cost, np.uint8)
    c = c[None] if c.ndim == 2 else c
    if c.ndim != 3 or not (1 <= c.shape[1] <= MAX_SIDE and 1 <= c.shape[2] <= MAX_SIDE):
        raise ValueError("gw and gh must be 1..4096")
    if c.shape[1] * c.shape[2] > MAX_AREA:
        raise ValueError("gw * gh must be at most 2^20")
    g = np.asarray(goals, np.int64).reshape(-1, 2)
    s = None if starts is None else np.asarray(starts, np.int64).reshape(-1, 2)
    if g.shape[0] != c.shape[0] or (s is not None and s.shape[0] != c.shape[0]):
        raise ValueError("one goal (and one start) per map is needed")
    return c, g, s


def _allowed(w, x, y, d, gw, gh):
    """the move between (x, y) and its neighbour d is allowed: both ends and, for a diagonal, both squeezed cells are passable
    (w: rows of Python ints, 0 = blocked); the rule is the same in both directions"""
    dx, dy = MOVES[d]
    ax, ay = x + dx, y + dy
    if not (0 <= ax < gw and 0 <= ay < gh) or not w[y][x] or not w[ay][ax]:
        return False
    return not (d & 1) or (w[y][ax] != 0 and w[ay][x] != 0)


def _potential(w, gw, gh, gx, gy):
    """Dijkstra from the goal over rows of Python ints -> rows of Python ints (INF: blocked or unreachable)"""
    P = [[INF] * gw for _ in range(gh)]
    if not (0 <= gx < gw and 0 <= gy < gh) or not w[gy][gx]:
        return P
    P[gy][gx] = 0
    heap = [(0, gx, gy)]
    while heap:
        pa, ax, ay = heapq.heappop(heap)
        if pa != P[ay][ax]:
            continue
        for d in range(8):
            if not _allowed(w, ax, ay, d, gw, gh):
                continue
            bx, by = ax + MOVES[d][0], ay + MOVES[d][1]
            cand = pa + (7 if d & 1 else 5) * w[by][bx]      # leaving b for a costs k * w(b)
            if cand < P[by][bx]:
                P[by][bx] = cand
                heapq.heappush(heap, (cand, bx, by))
    return P


def _walk(P, w, gw, gh, sx, sy):
    """the path from (sx, sy), whose P is finite -> the list of its cells"""
    cells, x, y = [(sx, sy)], sx, sy
    while P[y][x] != 0:
        best = None
        for d in range(8):
            if _allowed(w, x, y, d, gw, gh) and P[y + MOVES[d][1]][x + MOVES[d][0]] != INF:
                key = (P[y + MOVES[d][1]][x + MOVES[d][0]] + (7 if d & 1 else 5) * w[y][x], d)
                best = key if best is None or key < best else best
        if best is None or len(cells) > gw * gh:
            raise AssertionError("a finite cell without a finite neighbour")
        x, y = x + MOVES[best[1]][0], y + MOVES[best[1]][1]
        cells.append((x, y))
    return cells


def reference(cost, goals, starts, p: NavParams, potential=None, want_path: bool = True):
    """cost uint8 (gh, gw) or (n, gh, gw), goals (n, 2), starts (n, 2) or None -> (potential uint32 (n, gh, gw), path int32
    (n, max_path, 2) with -1 past the path's length (None without starts or with max_path == 0), stats uint32 (n, 5)).
    potential: a field to walk instead of the exact one (what a call with a fixed number of rounds left), uint32 (n, gh, gw).
    want_path=False: a call without the path output: no path, and no PATH_TRUNCATED, which is the flag of a path that was wanted
    (the length and P(start) are reported all the same)."""
    c, g, s = _prepare(cost, goals, starts, p)
    n, gh, gw = c.shape
    W = weights(c, p)
    pot = np.empty((n, gh, gw), np.uint32)
    path = np.full((n, p.max_path, 2), -1, np.int32) if s is not None and p.max_path > 0 and want_path else None
    stats = np.zeros((n, 5), np.uint32)
    for k in range(n):
        w = W[k].tolist()
        gx, gy = int(g[k, 0]), int(g[k, 1])
        P = _potential(w, gw, gh, gx, gy) if potential is None else np.asarray(potential[k], np.uint32).tolist()
        pot[k] = np.array(P, np.uint32)
        flags = 0
        if not (0 <= gx < gw and 0 <= gy < gh) or not w[gy][gx]:
            flags |= GOAL_BLOCKED
        length, p_start = 0, INF
        if s is not None:
            sx, sy = int(s[k, 0]), int(s[k, 1])
            if 0 <= sx < gw and 0 <= sy < gh:
                p_start = P[sy][sx]
            if p_start == INF:
                flags |= START_UNREACHABLE
            else:
                cells = _walk(P, w, gw, gh, sx, sy)
                length = len(cells)
                if path is not None:
                    path[k, :min(length, p.max_path)] = cells[:p.max_path]
                    if length > p.max_path:
                        flags |= PATH_TRUNCATED
        stats[k] = (flags, int((pot[k] != INF).sum()), length, p_start, int((W[k] == 0).sum()))
    return pot, path, stats


def loop_relaxation(cost, goal, p: NavParams) -> np.ndarray:
    """The header again for ONE map: P = INF but 0 at a passable goal, then sweeps of P(b) = min(P(b), P(a) + k * w(b)) over
    every cell and every allowed move, over Python integers, until a sweep changes nothing.  Shares nothing with reference but
    the weights' rule, which it restates.  -> uint32 (gh, gw).  Slow: small grids only."""
    c = np.asarray(cost, np.uint8)
    gh, gw = c.shape
    w = [[0] * gw for _ in range(gh)]
    for y in range(gh):
        for x in range(gw):
            v = int(c[y, x])
            if v == 255:
                w[y][x] = p.neutral + p.unknown_cost if p.flags & UNKNOWN_OK else 0
            elif v < p.lethal_cost:
                w[y][x] = p.neutral + v
    P = [[INF] * gw for _ in range(gh)]
    gx, gy = int(goal[0]), int(goal[1])
    if 0 <= gx < gw and 0 <= gy < gh and w[gy][gx]:
        P[gy][gx] = 0
    changed = True
    while changed:
        changed = False
        for y in range(gh):
            for x in range(gw):
                if not w[y][x]:
                    continue
                for d, (dx, dy) in enumerate(MOVES):
                    ax, ay = x + dx, y + dy
                    if not (0 <= ax < gw and 0 <= ay < gh) or not w[ay][ax] or P[ay][ax] == INF:
                        continue
                    if d & 1 and (not w[y][ax] or not w[ay][x]):
                        continue
                    cand = P[ay][ax] + (7 if d & 1 else 5) * w[y][x]
                    if cand < P[y][x]:
                        P[y][x], changed = cand, True
    return np.array(P, np.uint32)


def path_cost(path_cells, cost, p: NavParams) -> int:
    """the summed move costs of a path (a sequence of (x, y)): every move leaves its first cell"""
    W = weights(cost, p)
    total = 0
    for (x, y), (ax, ay) in zip(path_cells[:-1], path_cells[1:]):
        total += (7 if x != ax and y != ay else 5) * int(W[y, x])
    return total


# ---- the parameter file: one `key value` per line, `#` comments, as inflate.py's; goal and start take two values -----------------
_FILE = paramfile.spec(ints=_INTS, **{k: paramfile.Key(2, int) for k in _CELLS})


def save_params(path: str, p: NavParams) -> None:
    paramfile.write(path, "navigation function: costs 0..255; flags 1 = unknown cells are passable at unknown_cost; goal and start in cells (x y)",
                    _FILE, [(k, getattr(p, k)) for k in _INTS + _CELLS if getattr(p, k) is not None])


def load_params(path: str) -> NavParams:
    """A key that is missing keeps NavParams' default; an unknown or repeated key, or a wrong number of values, is an error."""
    return NavParams(**paramfile.read(path, _FILE))


# ---- what `filelist --plan` writes -------------------------------------------------------------------------------------------------
def scale_potential(potential: np.ndarray) -> np.ndarray:
    """uint32 (gh, gw) -> uint8: a finite P scaled to 0..254 by the largest finite one (integer division), INF cells at 255"""
    P = np.asarray(potential, np.uint32).astype(np.uint64)
    finite = P != INF
    top = int(P[finite].max()) if finite.any() else 0
    return np.where(finite, P * 254 // max(top, 1), 255).astype(np.uint8)


def write_pgm(path: str, potential: np.ndarray) -> None:
    g = np.ascontiguousarray(scale_potential(potential))
    with open(path, "wb") as f:
        f.write(f"P5\n{g.shape[1]} {g.shape[0]}\n255\n".encode() + g.tobytes())


def write_path(path: str, cells) -> None:
    """one `x y` line per cell of the path"""
    with open(path, "w") as f:
        for x, y in cells:
            f.write(f"{int(x)} {int(y)}\n")
