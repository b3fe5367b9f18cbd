"""The torus under the two rolling maps (``sn_costmap``, ``sn_elevation``): the pose quantiser and what a frame sees of the
window.  A window of mw x mh cells rolls with the pose: world cell (cx, cy) lives in slot (cx mod mw, cy mod mh), so slot (i, j)
under origin (ox, oy) holds world cell (ox + (i - ox) mod mw, oy + (j - oy) mod mh).  The vectorised twins (costmap.Reference,
elevation.Reference) use this; their LoopReference classes state the same rule on their own.  A "sub" is 1/256 of a cell.
"""
from __future__ import annotations

import math

import numpy as np

Q30 = 1 << 30


def pose_q(k256: float, mw: int, mh: int, pose) -> np.ndarray:
    """sn_costmap_pose_q / sn_elevation_pose_q: (x, y, yaw) -> int32 (6,) = {tx, ty, cq, sq, ox, oy} at k256 subs a metre.
    ValueError for a pose that is not finite or too far.  The library's may differ by one unit in cq, sq: two implementations
    of a double cos and sin."""
    x, y, yaw = (float(v) for v in pose)
    if not all(math.isfinite(v) for v in (x, y, yaw)) or abs(x * k256) > Q30 or abs(y * k256) > Q30:
        raise ValueError("the pose must be finite and within 2^30 subs of the origin")
    tx, ty = int(np.rint(x * k256)), int(np.rint(y * k256))
    return np.array([tx, ty, int(np.rint(math.cos(yaw) * Q30)), int(np.rint(math.sin(yaw) * Q30)), (tx >> 8) - mw // 2,
                     (ty >> 8) - mh // 2], np.int32)


def view(mw: int, mh: int, origin, prev):
    """What a frame with `origin` = (ox, oy) sees of the slots, after a frame with origin `prev` (None: a fresh stream) ->
    (cx int64 (mw,), cy int64 (mh,): the world cell of every slot column and row; moved bool (mh, mw): the slot held another
    world cell under `prev` and is forgotten (None without `prev`); rows (mh, 1), cols (1, mw): slot (i, j) is element
    [cy - oy][cx - ox] of the unrolled window)"""
    (ox, oy), i, j = origin, np.arange(mw, dtype=np.int64), np.arange(mh, dtype=np.int64)
    cx, cy = ox + (i - ox) % mw, oy + (j - oy) % mh
    moved = None
    if prev is not None:
        pox, poy = prev
        moved = (cy != poy + (j - poy) % mh)[:, None] | (cx != pox + (i - pox) % mw)[None, :]
    return cx, cy, moved, (cy - oy)[:, None], (cx - ox)[None, :]
