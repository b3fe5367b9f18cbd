"""The elevation map and its traversability verdict against float64 terrain geometry, on the numpy twin: render ->
elevation.Reference.push over the clip (-> inflate.reference -> navfn.reference), every assertion made against
tests/golden/terrain_truth.py (an analytic piecewise-planar terrain and a ray caster that share nothing with a twin) and none
against another twin.  What the stage tests cannot see is a convention that kernel, twin and loop got wrong together: the sign of
a yaw, the way z points, which of hi and lo the verdict subtracts, window cells against world cells.

The chain and the checks are shared with tests/test_gpu_terrain_truth.py, which feeds them what the kernels wrote.

Tolerances, all from the cell (c = 0.1 m), the map's depth step and the contract's roundings; none from an output:
  dZ    half a step of the map's integer at the farthest ray the map may use, Z^2 * 192000 / (fx * B) * out_scale / 2
        (terrain_truth.depth_half_step); a ray's hit moves by dZ times the ray's direction, whose horizontal part is at most
        HOR and whose vertical part is at most VER per unit of depth (the largest over the image, from the truth's rays);
  m     how far a hit may move in x and y: dZ * HOR + 2/256 c (the pose's rounding to 1/256 c per axis, and the rotation's)
        + 1e-5 m (fp32: 2^-23 of at most 8 m, a handful of operations);
  th    how far a height may move: dZ * VER + 1 mm (zmm = floor(zb * 1000)) + 1e-5 m.
A ray is "sure" of its cell where it keeps m from the cell's borders, from range_max_m and from z_min_m / z_max_m.  Per frame a
cell certainly fuses where it has min_points sure rays, and may fuse where it has min_points rays in all (a ray counts for every
cell within m of it).  Fusion with any alpha keeps hi between the extremes of the frames' maxima and lo between those of the
minima (the blend's rounding never passes either end), so after the clip, for a cell that certainly fused at least once and has
not left the window since:
  hi lies in [the least (highest sure ray - th) over the frames that may have fused, the greatest (highest ray + th)],
  lo in [the least (lowest ray - th), the greatest (lowest sure ray + th)];
a cell that never had min_points rays is unknown; the rest (a frame that may have fused without sure rays enough) is left out.
From those intervals: a cell is certainly lethal where some certainly known neighbour (or itself) has hi_lb(n) - lo_ub(c) or
hi_lb(c) - lo_ub(n) above max_step_mm, certainly free where every neighbour that may be known has both hi_ub - lo_lb at or under
it.  The cells left out are at most a fifth of those that received any ray (chain truth's cap); the measured shares are in
profiles/terrain_truth.txt.
  far   a lethal cell has, within its neighbourhood, two points whose heights differ by more than max_step_mm; the terrain
        between them is continuous but for its faces and rises by at most (radius + 1) c tan(7 deg) + 2 th < max_step_mm, so a
        face crosses the segment between them: the cell's centre lies within sqrt(2) (radius + 1/2) c + m of a face.
  ramp  a ramp cell (radius + 1) cells clear of the ramp's ends has only ramp in its neighbourhood: rise <= (radius + 1) c
        tan(7 deg) + 2 th + m tan(7 deg) = 27.4 mm <= max_step_mm = 50, so it is 0 wherever it is known.
"""
import dataclasses
import functools
import math

import numpy as np
import pytest

import terrain_truth as tt
import test_chain_truth as ct
from hobot_stereonet_amd import api, inflate, navfn, obstacles
from hobot_stereonet_amd import elevation as el
from hobot_stereonet_amd.elevation import ElevationParams
from hobot_stereonet_amd.inflate import InflateParams
from hobot_stereonet_amd.navfn import NavParams

CAM, W, H = tt.CAM, tt.W, tt.H
CELL = float(np.float32(0.1))
RANGE, Z_BAND, MIN_POINTS, MAX_STEP, RADIUS = 3.5, (-1.0, 1.0), 2, 50, 1
SQ2 = math.sqrt(2.0)
IP = InflateParams(cell_m=CELL, inscribed_radius_m=0.2, inflation_radius_m=0.4, cost_scaling=3.0, lethal_min=100, flags=0)
NAV_OK = NavParams(neutral=50, lethal_cost=253, unknown_cost=0, flags=navfn.UNKNOWN_OK, max_rounds=0, max_path=400)
NAV_STRICT = dataclasses.replace(NAV_OK, flags=0)
# the mistakes run_map can make on this side of the stage, and the check that must catch each
CAUGHT_BY = {"yaw negated": "heights", "the mount's z negated": "heights", "hi and lo swapped in the verdict": "lethal",
             "window cells taken as world cells": "known"}
# a region of world cells that holds every window of every clip: the truth's arrays are [cy - GY][cx - GX]
GX, GY, GW, GH = -60, -60, 160, 120


def params(t):
    return ElevationParams(mw=t.window[0], mh=t.window[1], cell_m=CELL, base_from_cam=tt.mount(t), z_min_m=Z_BAND[0], z_max_m=Z_BAND[1],
                           range_max_m=RANGE, min_points=MIN_POINTS, alpha=128, max_step_mm=MAX_STEP, radius=RADIUS)


@functools.lru_cache(maxsize=None)
def truth(name):
    """-> what terrain_truth alone says about the final map of a scene's clip (see the module's docstring)"""
    t = tt.SCENES[name]
    mw, mh = t.window
    _, d = tt.camera_rays(t, (0.0, 0.0, 0.0))
    hor, ver = float(np.hypot(d[..., 0], d[..., 1]).max()), float(np.abs(d[..., 2]).max())
    z_far = max(float(tt.frame_rays(t, p, CELL, RANGE, Z_BAND, 0.01)[2].max()) for p in t.poses)
    dz = float(tt.depth_half_step(z_far))
    m, th = dz * hor + 2.0 / 256.0 * CELL + 1e-5, dz * ver + 1e-3 + 1e-5
    shape = (GH, GW)
    status = np.zeros(shape, np.int8)                     # 0 certainly unknown, 1 certainly known, 2 left out
    hi_lb, hi_ub, lo_lb, lo_ub = (np.full(shape, v) for v in (np.inf, -np.inf, np.inf, -np.inf))
    any_ray = np.zeros(shape, bool)
    origins = [tt.window_origin(p, CELL, mw, mh) for p in t.poses]
    jj, ii = np.meshgrid(np.arange(GH) + GY, np.arange(GW) + GX, indexing="ij")
    for pose, (ox, oy) in zip(t.poses, origins):
        inside = (ii >= ox) & (ii < ox + mw) & (jj >= oy) & (jj < oy + mh)
        assert GX <= ox and ox + mw <= GX + GW and GY <= oy and oy + mh <= GY + GH
        for a, v in ((hi_lb, np.inf), (hi_ub, -np.inf), (lo_lb, np.inf), (lo_ub, -np.inf)):
            a[~inside] = v
        status[~inside], any_ray[~inside] = 0, False
        c, z, _, sure, cands = tt.frame_rays(t, pose, CELL, RANGE, Z_BAND, m)
        s_cnt, s_max, s_min = np.zeros(shape, np.int64), np.full(shape, -np.inf), np.full(shape, np.inf)
        a_cnt, a_max, a_min = np.zeros(shape, np.int64), np.full(shape, -np.inf), np.full(shape, np.inf)
        at = (c[sure, 1] - GY, c[sure, 0] - GX)
        np.add.at(s_cnt, at, 1), np.maximum.at(s_max, at, z[sure]), np.minimum.at(s_min, at, z[sure])
        for r in range(len(z)):
            for cx, cy in {(int(a), int(b)) for a, b in cands[r]}:
                a_cnt[cy - GY, cx - GX] += 1
                a_max[cy - GY, cx - GX], a_min[cy - GY, cx - GX] = max(a_max[cy - GY, cx - GX], z[r]), min(a_min[cy - GY, cx - GX], z[r])
        may, certain = inside & (a_cnt >= MIN_POINTS), inside & (s_cnt >= MIN_POINTS)
        any_ray |= inside & (a_cnt > 0)
        # a frame that certainly fused: its maximum is at least its highest sure ray and at most its highest ray, its minimum likewise
        f_hi_lb, f_lo_ub = np.where(certain, s_max, a_min) - th, np.where(certain, s_min, a_max) + th
        hi_lb[may], hi_ub[may] = np.minimum(hi_lb, f_hi_lb)[may], np.maximum(hi_ub, a_max + th)[may]
        lo_lb[may], lo_ub[may] = np.minimum(lo_lb, a_min - th)[may], np.maximum(lo_ub, f_lo_ub)[may]
        status[certain & (status == 0)] = 1
        status[may & ~certain & (status == 0)] = 2
    ox, oy = origins[-1]
    win = (slice(oy - GY, oy - GY + mh), slice(ox - GX, ox - GX + mw))
    T = dict(t=t, dz=dz, m=m, th=th, origin=(ox, oy), origins=origins, status=status[win], any_ray=any_ray[win], hi_lb=hi_lb[win] * 1000.0,
             hi_ub=hi_ub[win] * 1000.0, lo_lb=lo_lb[win] * 1000.0, lo_ub=lo_ub[win] * 1000.0, centres=tt.cell_centres((ox, oy), CELL, mw, mh))
    # the verdict's intervals: the neighbourhood clipped to the window
    known, maybe = T["status"] == 1, T["status"] != 0
    pad = lambda a, v: np.pad(a, RADIUS, constant_values=v)      # noqa: E731
    n_hi_lb, n_lo_ub = pad(np.where(known, T["hi_lb"], -np.inf), -np.inf), pad(np.where(known, T["lo_ub"], np.inf), np.inf)
    n_hi_ub, n_lo_lb = pad(np.where(maybe, T["hi_ub"], -np.inf), -np.inf), pad(np.where(maybe, T["lo_lb"], np.inf), np.inf)
    c_hi_lb, c_lo_ub = np.where(known, T["hi_lb"], -np.inf), np.where(known, T["lo_ub"], np.inf)
    c_hi_ub, c_lo_lb = np.where(maybe, T["hi_ub"], -np.inf), np.where(maybe, T["lo_lb"], np.inf)
    sure_rise, most_rise = np.full((mh, mw), -np.inf), np.full((mh, mw), -np.inf)
    for dy in range(2 * RADIUS + 1):
        for dx in range(2 * RADIUS + 1):
            w = (slice(dy, dy + mh), slice(dx, dx + mw))
            sure_rise = np.maximum(sure_rise, np.maximum(n_hi_lb[w] - c_lo_ub, c_hi_lb - n_lo_ub[w]))
            most_rise = np.maximum(most_rise, np.maximum(n_hi_ub[w] - c_lo_lb, c_hi_ub - n_lo_lb[w]))
    T["must_lethal"] = known & (sure_rise > MAX_STEP)
    T["must_free"] = known & (most_rise <= MAX_STEP)      # a neighbour that is left out counts with its widest interval
    return T


# ---- the stage ---------------------------------------------------------------------------------------------------------------------
class Twins:
    def elevation(self, p, poses, raws):
        q = api.elevation_pose_q(p, poses)
        trav, hi, lo, rise, stats = el.Reference(p).push(q, raws, CAM)
        return trav, hi, lo, rise, stats, q

    def inflate(self, grid, ip):
        return inflate.reference(grid, ip, api.inflate_table(ip))[0]

    def navfn(self, cost, goals, starts, nav):
        return navfn.reference(cost, goals, starts, nav)


def world_cell(xy):
    return int(math.floor(xy[0] / CELL)), int(math.floor(xy[1] / CELL))


def run_map(t, be, mistake=None):
    """The clip of a scene through the stage on a backend -> a dict of what it made.  `mistake` applies one of CAUGHT_BY's on
    this side of the stage: to what it is handed or to how its outputs are read, never to the stage."""
    assert mistake is None or mistake in CAUGHT_BY, mistake
    poses = np.asarray(t.poses, np.float64)
    raws = np.stack([tt.render(t, p) for p in poses])
    p = params(t)
    if mistake == "yaw negated":
        poses = poses * (1, 1, -1)
    if mistake == "the mount's z negated":
        p = dataclasses.replace(p, base_from_cam=tuple(float(v) for v in np.asarray(p.base_from_cam) * ([1] * 8 + [-1] * 4)))
    trav, hi, lo, rise, stats, q = be.elevation(p, poses, raws)
    R = dict(raws=raws, trav=trav, hi=hi, lo=lo, rise=rise, stats=stats, q=np.asarray(q), origin=(int(q[-1][4]), int(q[-1][5])), p=p)
    if mistake == "hi and lo swapped in the verdict":
        R["trav"] = np.stack([el.verdict(p, l, h)[0] for h, l in zip(hi, lo)])
    if mistake == "window cells taken as world cells":
        R["origin"] = (0, 0)
    return R


def at_truth(name, R, plane):
    """the final frame's plane re-read at the truth's window: element [j][i] is the world cell (ox + i, oy + j) of the truth's
    origin, whatever origin the stage reported; cells the stage's window does not hold read as None (masked)"""
    T = truth(name)
    mw, mh = T["t"].window
    (ox, oy), (rx, ry) = T["origin"], R["origin"]
    out = np.ma.masked_all((mh, mw), dtype=np.int64)
    i0, i1, j0, j1 = max(ox, rx), min(ox, rx) + mw, max(oy, ry), min(oy, ry) + mh
    if i0 < i1 and j0 < j1:
        out[j0 - oy:j1 - oy, i0 - ox:i1 - ox] = plane[j0 - ry:j1 - ry, i0 - rx:i1 - rx]
    return out


def check_known(name, R, tag="terrain_truth"):
    """every cell that certainly fused is known, every cell that never had min_points rays is unknown; the window's origin is the
    cell of the pose less half the window"""
    T = truth(name)
    hi = at_truth(name, R, R["hi"][-1]).filled(el.UNKNOWN)
    known = hi != el.UNKNOWN
    sure, none, rays = T["status"] == 1, T["status"] == 0, int(T["any_ray"].sum())
    share = float((T["status"] == 2).sum()) / rays
    print(f"{tag} {name} | known | {int(sure.sum())} cells certainly known, {int((sure & ~known).sum())} of them unknown | {int((none & known).sum())} known "
          f"cells without {MIN_POINTS} rays | left out {share:.3f} <= 0.2 of {rays} cells with a ray | m {T['m'] * 1e3:.2f} mm, th {T['th'] * 1e3:.2f} mm")
    assert R["origin"] == T["origin"], (R["origin"], T["origin"])
    assert sure.sum() >= 300 and share <= 0.2, (int(sure.sum()), share)
    assert not (sure & ~known).any() and not (none & known).any()


def check_heights(name, R, tag="terrain_truth"):
    """a known cell's lo and hi lie within the terrain's own minimum and maximum over the cell (widened by m; faces count up to
    z_max_m), widened by th; and where the cell is certainly known, within the intervals of its rays"""
    T = truth(name)
    hi, lo = at_truth(name, R, R["hi"][-1]).filled(el.UNKNOWN), at_truth(name, R, R["lo"][-1]).filled(el.UNKNOWN)
    known = hi != el.UNKNOWN
    zmin, zmax = tt.height_range(T["t"], T["centres"] - CELL / 2 - T["m"], T["centres"] + CELL / 2 + T["m"], Z_BAND[1])
    th = T["th"] * 1e3
    below, above = (zmin * 1e3 - th) - lo, hi - (zmax * 1e3 + th)
    worst = float(max(below[known].max(), above[known].max(), (lo - hi)[known].max())) if known.any() else -np.inf
    sure = known & (T["status"] == 1)
    tight = float(max((T["hi_lb"] - hi)[sure].max(), (hi - T["hi_ub"])[sure].max(), (T["lo_lb"] - lo)[sure].max(), (lo - T["lo_ub"])[sure].max())) if sure.any() else -np.inf
    print(f"{tag} {name} | heights | {int(known.sum())} known cells, furthest outside the terrain's range over the cell {worst:.3f} mm <= 0 | "
          f"{int(sure.sum())} certainly known, furthest outside their rays' intervals {tight:.3f} mm <= 0")
    assert known.sum() >= 300 and worst <= 0 and tight <= 0, (worst, tight)


def check_lethal(name, R, tag="terrain_truth"):
    """certainly lethal cells are 100, certainly free cells 0; a cell that holds a face higher than max_step_mm and is certainly
    known with both levels in its rays is among the former; no lethal cell lies further than `far` from a face"""
    T = truth(name)
    t = T["t"]
    trav = at_truth(name, R, R["trav"][-1]).filled(-1)
    faces = tt.face_segments(t, MAX_STEP / 1000.0)
    face_cells = tt.dist_to_segments(faces, T["centres"]) <= CELL / 2 if len(faces) else np.zeros(trav.shape, bool)      # Chebyshev would be exact; faces run along the axes
    lethal = trav == 100
    far = SQ2 * (RADIUS + 0.5) * CELL + T["m"]
    reach = float(tt.dist_to_segments(faces, T["centres"][lethal]).max()) if lethal.any() else 0.0
    rays = int(T["any_ray"].sum())
    decided = T["must_lethal"] | T["must_free"] | (T["status"] == 0)      # a cell that is certainly unknown is -1: check_known
    share = float((T["any_ray"] & ~decided).sum()) / rays
    print(f"{tag} {name} | lethal | {int(lethal.sum())} lethal cells, furthest from a face {reach:.4f} m <= {far:.4f} m | certainly lethal "
          f"{int(T['must_lethal'].sum())} ({int((T['must_lethal'] & face_cells).sum())} hold a face), not 100: {int((T['must_lethal'] & ~lethal).sum())} | certainly free "
          f"{int(T['must_free'].sum())}, not 0: {int((T['must_free'] & (trav != 0)).sum())} | left out {share:.3f} <= 0.2 of {rays} cells with a ray")
    assert share <= 0.2, share
    assert not (T["must_lethal"] & ~lethal).any() and not (T["must_free"] & (trav != 0)).any()
    assert reach <= far, (reach, far)
    if len(faces) and t.pitch == 0.0:      # a face seen from its foot: cells that hold it are certainly lethal
        assert (T["must_lethal"] & face_cells).sum() >= 5
    if not len(faces):
        assert not lethal.any()


def check_ramp(name, R, tag="terrain_truth"):
    """every ramp cell clear of the ramp's ends is 0 wherever it is known, and enough of them are certainly known"""
    T = truth(name)
    t = T["t"]
    if t.ramp is None:
        return
    trav = at_truth(name, R, R["trav"][-1]).filled(-1)
    x = T["centres"][..., 0]
    inner = (x - CELL / 2 >= t.ramp[0] + (RADIUS + 1) * CELL) & (x + CELL / 2 <= t.ramp[1] - (RADIUS + 1) * CELL)
    known = inner & (trav != -1)
    bound = ((RADIUS + 1) * CELL + T["m"]) * tt.RAMP_TAN * 1e3 + 2 * T["th"] * 1e3
    rise = at_truth(name, R, R["rise"][-1]).filled(0)
    print(f"{tag} {name} | ramp | {int(known.sum())} known ramp cells clear of its ends ({int((inner & (T['status'] == 1)).sum())} certainly), "
          f"{int((known & (trav != 0)).sum())} not free | largest rise {int(rise[known].max()) if known.any() else 0} mm <= {bound:.1f} mm <= {MAX_STEP} mm")
    assert bound <= MAX_STEP and (inner & (T["status"] == 1)).sum() >= 40
    assert not (known & (trav != 0)).any() and rise[known].max() <= bound


def check_flood(name, R, tag="terrain_truth"):
    """a flood fill (8-connected) from the robot's cell over trav == 0 reaches no cell beyond the edge or kerb; unknown is blocked.
    The robot's cell is free (the clip's first frames saw it), and there are free cells beyond the line to be reached."""
    T = truth(name)
    t = T["t"]
    if t.edge_x is None:
        return
    trav = at_truth(name, R, R["trav"][-1]).filled(-1)
    mw, mh = t.window
    sx, sy = world_cell(t.poses[-1])
    si, sj = sx - T["origin"][0], sy - T["origin"][1]
    free = trav == 0
    beyond = T["centres"][..., 0] - CELL / 2 >= t.edge_x
    seen = np.zeros(free.shape, bool)
    stack = [(sj, si)] if free[sj, si] else []
    while stack:
        j, i = stack.pop()
        if seen[j, i]:
            continue
        seen[j, i] = True
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                a, b = j + dj, i + di
                if 0 <= a < mh and 0 <= b < mw and free[a, b] and not seen[a, b]:
                    stack.append((a, b))
    print(f"{tag} {name} | flood | {int(seen.sum())} cells reached from the robot's cell, {int((seen & beyond).sum())} beyond x = {t.edge_x} m | "
          f"{int((free & beyond).sum())} free cells beyond")
    assert free[sj, si] and seen.sum() >= 50, "the robot's cell is not free"
    assert (free & beyond).sum() >= 20, "nothing free beyond the line: the check is empty"
    assert not (seen & beyond).any()


CHECKS = {"known": check_known, "heights": check_heights, "lethal": check_lethal, "ramp": check_ramp, "flood": check_flood}


def failures(name, R, checks=CHECKS):
    out = {}
    for label, fn in checks.items():
        try:
            fn(name, R)
        except AssertionError as e:
            out[label] = str(e)[:200]
    return out


def check_plan(name, R, be, tag="terrain_truth"):
    """trav -> inflation -> navigation function.  The ramp: a path from the robot's cell to the goal on top of it, over ramp cells,
    through no lethal cell.  The drop: with unknown cells blocked there is no route to the goal on the lower floor, although
    the goal's cell itself is open."""
    T = truth(name)
    t = T["t"]
    ox, oy = R["origin"]
    cost = be.inflate(R["trav"][-1:], IP)
    (gx, gy), (sx, sy) = world_cell(t.goal), world_cell(t.poses[-1])
    goal, start = (gx - ox, gy - oy), (sx - ox, sy - oy)
    if t.ramp is not None:
        pot, path, stats = be.navfn(cost, [goal], [start], NAV_OK)[:3]
        n = int(stats[0][2])
        cells = path[0][:n].astype(np.int64)
        on_ramp = ((cells[:, 0] + ox + 0.5) * CELL > t.ramp[0]) & ((cells[:, 0] + ox + 0.5) * CELL < t.ramp[1])
        print(f"{tag} {name} | plan | flags {int(stats[0][0])}, {n} cells from {start} to {goal}, {int(on_ramp.sum())} of them on the ramp")
        assert stats[0][0] == 0 and tuple(cells[0]) == start and tuple(cells[-1]) == goal and on_ramp.sum() >= 10
        assert not (R["trav"][-1][cells[:, 1], cells[:, 0]] == 100).any()
    else:
        pot, path, stats = be.navfn(cost, [goal], [start], NAV_STRICT)[:3]
        print(f"{tag} {name} | plan | flags {int(stats[0][0])} (start unreachable = {navfn.START_UNREACHABLE}), cost at the start {int(cost[0][start[1], start[0]])}, "
              f"at the goal {int(cost[0][goal[1], goal[0]])}")
        assert cost[0][goal[1], goal[0]] < 253 and cost[0][start[1], start[0]] < 253, "the goal or the start is not open: the check is empty"
        assert stats[0][0] == navfn.START_UNREACHABLE


def check_old_chain(name, tag="terrain_truth"):
    """what the feature fixes: sn_obstacles_from_raw's flat-floor rule under the chain truth's parameters reads the upper part of
    the ramp as obstacles, and reads nothing at all at the drop (no cell occupied, the floor beyond it unknown)"""
    t = tt.SCENES[name]
    op = dataclasses.replace(ct.OP, base_from_cam=tt.mount(t))
    raws = np.stack([tt.render(t, p) for p in t.poses])
    occ = obstacles.reference(raws, CAM, op, api.beam_edges(op))[0]
    gx0, gy0 = ct.GRID[0], ct.GRID[1]
    ix, iy = np.meshgrid(np.arange(op.gw), np.arange(op.gh))
    base = np.stack([gx0 + (ix + 0.5) * CELL, gy0 + (iy + 0.5) * CELL], -1)
    x, y, yaw = t.poses[-1]
    wx = x + math.cos(yaw) * base[..., 0] - math.sin(yaw) * base[..., 1]
    if t.ramp is not None:
        upper = (wx > t.ramp[0] + (ct.Z_BAND[0] + 0.01) / tt.RAMP_TAN + CELL) & (wx < t.ramp[1])
        print(f"{tag} {name} | old chain | {int((occ[-1] == 100)[upper].sum())} occupied cells on the upper ramp, {int((occ[-1] == 0)[upper].sum())} free")
        assert (occ[-1] == 100)[upper].sum() >= 20 and not (occ[-1] == 0)[upper].any()
    else:
        beyond = wx > t.edge_x + CELL
        print(f"{tag} {name} | old chain | {int((occ == 100).sum())} occupied cells in the whole clip, {int((occ[-1] != -1)[beyond].sum())} known cells beyond the edge")
        assert not (occ == 100).any() and not (occ[-1] != -1)[beyond].any()


def check_mirror(a, b, Ra, Rb, tag="terrain_truth"):
    """each lethal cell of either final map has a lethal cell of the other, flipped in y, within one cell; likewise the known cells"""
    out = []
    for what, pick in (("lethal", lambda R: R["trav"][-1] == 100), ("known", lambda R: R["hi"][-1] != el.UNKNOWN)):
        def cells(R):
            j, i = np.nonzero(pick(R))
            return np.stack([i + R["origin"][0], j + R["origin"][1]], -1)
        A, B = cells(Ra), cells(Rb) * (1, -1) - (0, 1)
        if len(A) == 0 and len(B) == 0:
            out.append(f"no {what} cells")
            continue
        assert len(A) and len(B), what
        gap = np.abs(A[:, None, :] - B[None, :, :]).max(-1)
        out.append(f"{len(A)} and {len(B)} {what} cells, furthest from its image {int(max(gap.min(1).max(), gap.min(0).max()))} <= 1 cell")
        assert gap.min(1).max() <= 1 and gap.min(0).max() <= 1, what
    print(f"{tag} {a} | mirror | " + " | ".join(out))


@functools.lru_cache(maxsize=None)
def twin_map(name):
    """the twin's map of a scene, computed once, shared and never changed"""
    R = run_map(tt.SCENES[name], Twins())
    for v in R.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return R


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
def test_the_scenes_are_what_they_claim():
    """from terrain_truth alone: the mirrored image is the mirror image, the depth relation gives back the floor, the height
    function and the ray caster agree, patches meet at faces or continuously, the ramp is 7 degrees"""
    for t in tt.BASE:
        m = tt.SCENES[t.name + " mirrored"]
        for pa, pb in zip(t.poses, m.poses):
            assert np.array_equal(tt.render(t, pa), tt.render(m, pb)[:, ::-1]), t.name
        pts, label, depth = tt.hit_points(t, t.poses[0])
        g = label == tt.GROUND
        assert g.sum() > 2000 and np.abs(tt.height(t, pts[g][:, :2]) - pts[g][:, 2]).max() < 1e-9, t.name
        for x0, y0, x1, y1, zl, zh in t.faces:      # a face joins the heights of the ground on its two sides (a wall stands on it)
            mid = np.array([(x0 + x1) / 2, (y0 + y1) / 2])
            sides = [float(tt.height(t, mid + e)) for e in ((-1e-6, 0.0), (1e-6, 0.0))]
            assert min(sides) == pytest.approx(zl, abs=1e-6) and (max(sides) == pytest.approx(zh, abs=1e-6) or t is tt.FLAT_WALL), t.name
    assert 6.0 <= math.degrees(math.atan(tt.RAMP_TAN)) <= 8.0 and tt.height(tt.RAMP, (3.0, 0.0)) == pytest.approx(tt.RAMP_TOP)
    assert tt.height(tt.RAMP, (2.4, 1.0)) == pytest.approx(0.6 * tt.RAMP_TAN) and tt.height(tt.DROP, (2.6, 0.0)) == -0.3 and tt.height(tt.KERB, (2.3, 0.0)) == 0.06 and tt.height(tt.KERB, (2.2, 0.0)) == 0.0
    raw = tt.render(tt.FLAT_WALL, (0.0, 0.0, 0.0))
    assert raw[63, 50] == round(80.0 * 120.0 / (0.5 * 80.0 / 42.5 * 192000.0) / 2.60443857769133e-6)       # the ground under row 63
    zmin, zmax = tt.height_range(tt.KERB, np.array([2.2, 0.0]), np.array([2.3, 0.1]))
    assert (zmin, zmax) == (0.0, 0.06)
    zmin, zmax = tt.height_range(tt.RAMP, np.array([2.0, 0.0]), np.array([2.1, 0.1]))
    assert zmin == pytest.approx(0.2 * tt.RAMP_TAN) and zmax == pytest.approx(0.3 * tt.RAMP_TAN)


@pytest.mark.parametrize("name", list(tt.SCENES))
def test_the_map_against_the_truth(name):
    bad = failures(name, twin_map(name))
    assert not bad, bad


@pytest.mark.parametrize("name", ["ramp", "ramp mirrored", "drop", "drop mirrored"])
def test_what_the_feature_fixes_and_the_chain_through(name):
    check_old_chain(name)
    check_plan(name, twin_map(name), Twins())


@pytest.mark.parametrize("name", [t.name for t in tt.BASE])
def test_the_mirrored_world(name):
    check_mirror(name, name + " mirrored", twin_map(name), twin_map(name + " mirrored"))


@pytest.mark.parametrize("mistake", list(CAUGHT_BY))
def test_every_mistake_is_caught(mistake):
    """the checks have teeth: each convention got wrong on this side of the stage fails the check that is there for it"""
    R = run_map(tt.KERB, Twins(), mistake)
    bad = failures("kerb", R)
    print(f"terrain_truth kerb | mistake | {mistake}: caught by {sorted(bad)}")
    assert CAUGHT_BY[mistake] in bad, (mistake, bad)
