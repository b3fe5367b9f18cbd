"""The chain from the map to the command against float64 scene geometry, on the numpy twins: render -> obstacles.reference ->
costmap.Reference.push over the clip -> inflate.reference -> navfn.reference -> rollout.reference, every assertion made against
tests/golden/scene_truth.py (an analytic world and a ray caster that share nothing with a twin) and none against another twin.
What the stage tests cannot see is a convention that kernel, twin and loop got wrong together: the way y points, the sign of a
yaw, the corner the window's origin names, window cells against world cells, the side an arc turns to, the way a ray clears.

The chain and the checks are shared with tests/test_gpu_chain_truth.py, which feeds them what the kernels wrote.  Each check_*
reads the api's arrays and hands cell centres in metres and values to a *_bounds function that holds the assertions;
tests/test_node_truth.py hands the same functions what it decoded from the node's messages.

Tolerances, all from the cell (c = 0.1 m), the map's depth step and the contracts' roundings; none from an output:
  dZ    half a step of the map's integer at the farthest wall ray of the scene, Z^2 * 192000 / (fx * B) * out_scale / 2;
  E     for the scene whose mount comes from the ground fit only: Z_max * 2e-3 + 5e-3 * height, the angle and height bounds
        that test_ground.py::test_geometric_truth_on_seeded_scenes asserts, added to every position tolerance of that scene;
  grid  an occupied cell holds a hit point: its centre lies within sqrt(2)/2 c + dZ of a wall;
  map   a costmap cell's centre falls in an occupied base cell (diagonal sqrt(2) c) under a pose rounded to 1/256 c:
        D = sqrt(2) c + dZ + 2/256 c from a seen wall point, and every seen wall point has an occupied cell within D;
  cost  a cell below 253 has no occupied cell within the inscribed radius r, so it keeps r - (sqrt(2)/2 + sqrt(2)) c - dZ from
        every seen wall point, and a cell within that of one is at 253 or 254;
  arc   see check_rollout.
"""
import dataclasses
import functools
import math

import numpy as np
import pytest

import scene_truth as st
from hobot_stereonet_amd import api, costmap, ground, inflate, navfn, obstacles, rollout
from hobot_stereonet_amd.costmap import CostmapParams
from hobot_stereonet_amd.ground import GroundParams
from hobot_stereonet_amd.inflate import InflateParams
from hobot_stereonet_amd.navfn import NavParams
from hobot_stereonet_amd.obstacles import ObstacleParams
from hobot_stereonet_amd.rollout import RolloutParams

CAM, W, H = st.CAM, st.W, st.H
CELL = float(np.float32(0.1))                  # the structs hold fp32
Z_BAND = (0.1, 1.5)                            # z_lo_m, z_hi_m: the heights the obstacle stage counts as an obstacle
MIN_HITS = 3
GRID = (0.0, -4.0, CELL, 60, 80)               # x_min, y_min, cell, gw, gh: not square
SQ2 = math.sqrt(2.0)
# the level mount written out from the frames: x = Z, y = -X, z = -Y, the camera 0.5 m up
LEVEL = (0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.5)
OP = ObstacleParams(base_from_cam=LEVEL, x_min_m=GRID[0], y_min_m=GRID[1], cell_m=CELL, gw=GRID[3], gh=GRID[4], z_floor_m=-0.15, z_lo_m=Z_BAND[0],
                    z_hi_m=Z_BAND[1], min_obstacle_hits=MIN_HITS, min_ground_hits=3, beams=26, angle_min_rad=-0.52, angle_increment_rad=0.04,
                    range_min_m=0.0, range_max_m=8.0)
# one hit outlasts the misses of a whole clip (11 * 10 < 120): a cell seen occupied once is occupied at the end
CP = CostmapParams(mw=100, mh=100, l_hit=120, l_miss=10, l_min=-200, l_max=350, clear_margin_m=0.1, clear_min_m=0.0, clear_max_m=0.0)
# the grid value of log-odds 1 by the costmap's contract, ((L - l_min) * 100 + span / 2) / span: "occupied" is L > 0
LETHAL_MIN = ((1 - CP.l_min) * 100 + (CP.l_max - CP.l_min) // 2) // (CP.l_max - CP.l_min)
assert LETHAL_MIN == 37 and ((0 - CP.l_min) * 100 + (CP.l_max - CP.l_min) // 2) // (CP.l_max - CP.l_min) == 36
INSCRIBED, INFLATION = 0.4, 0.8                # 4 and 8 cells
IP = InflateParams(cell_m=CELL, inscribed_radius_m=INSCRIBED, inflation_radius_m=INFLATION, cost_scaling=3.0, lethal_min=LETHAL_MIN, flags=0)
NAV = NavParams(neutral=50, lethal_cost=253, unknown_cost=0, flags=navfn.UNKNOWN_OK, max_rounds=0, max_path=400)
RP = RolloutParams(cell_m=CELL, v_min=0.0, v_max=0.5, nv=5, w_min=-1.0, w_max=1.0, nw=11, sim_time_s=3.0, steps=15, lethal_cost=254,
                   centre_lethal_cost=253, unknown_cost=0, flags=rollout.UNKNOWN_OK, w_goal=1, w_occ=1)
# the outline of a 0.4 m x 0.3 m robot every 0.1 m: 14 points, x ahead, y to the left
FOOTPRINT = np.array([(0.2 - 0.1 * i, 0.15) for i in range(4)] + [(-0.2, 0.15 - 0.1 * i) for i in range(3)] +
                     [(-0.2 + 0.1 * i, -0.15) for i in range(4)] + [(0.2, -0.15 + 0.1 * i) for i in range(3)], np.float32)
GP = GroundParams(hypotheses=128, refits=2, tol_px=0.02, min_inliers=50, min_area=16)      # test_ground.py's, whose bounds E takes
FIT_ANGLE, FIT_HEIGHT = 2e-3, 5e-3                                                      # rad, and a share of the height
# the mistakes run_chain can make on this side of the chain, and the check that must catch each
CAUGHT_BY = {"yaw negated for the costmap": "costmap", "yaw negated for the rollout": "rollout", "the obstacle grid flipped in y": "grid",
             "the mount's y taken as +X": "grid", "the rollout's origin left at (0, 0)": "rollout", "the goal cell without the window origin": "path",
             "gw and gh swapped": "costmap", "the truth arc with -w": "rollout"}


def costmap_params(scene):
    return dataclasses.replace(CP, mw=scene.window[0], mh=scene.window[1])


# ---- what the truth alone says about a scene --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def truth(name):
    """-> the figures of a scene that every check shares, from scene_truth alone"""
    scene = st.SCENES[name]
    mw, mh = scene.window
    z_max = 0.0
    for pose in scene.poses:
        _, _, _, depth = st.wall_rays(scene, pose, GRID, Z_BAND)
        z_max = max(z_max, float(depth.max()))
    dz = st.depth_half_step(z_max)
    fit = z_max * FIT_ANGLE + FIT_HEIGHT * scene.cam_height if scene.fitted_mount else 0.0
    tol = dz + fit
    origins = [st.window_origin(p, CELL, mw, mh) for p in scene.poses]
    band_wide = (Z_BAND[0] - 1e-3 * CELL - fit, Z_BAND[1] + 1e-3 * CELL + fit)
    band_sure = (Z_BAND[0] + 1e-3 * CELL + fit, Z_BAND[1] - 1e-3 * CELL - fit)
    any_ray, sure = [], []
    for k, pose in enumerate(scene.poses):
        # a point counts for the final map where its world cell lies inside the window from frame k to the last
        def stays(xy):
            c = np.floor(xy / CELL).astype(np.int64)
            ok = np.ones(len(xy), bool)
            for ox, oy in origins[k:]:
                ok &= (c[:, 0] >= ox) & (c[:, 0] < ox + mw) & (c[:, 1] >= oy) & (c[:, 1] < oy + mh)
            return xy[ok]
        any_ray.append(stays(st.seen_wall(scene, [pose], 1, GRID, band_wide)))
        sure.append(stays(st.seen_wall(scene, [pose], MIN_HITS + 2, GRID, band_sure)))
    out = dict(scene=scene, z_max=z_max, dz=dz, fit=fit, tol=tol, origins=origins, any_ray=np.concatenate(any_ray), sure=np.concatenate(sure),
               segs=st.segments(scene), D=SQ2 * CELL + tol + 2.0 / 256.0 * CELL, clear=INSCRIBED - (SQ2 / 2 + SQ2) * CELL - tol)
    assert out["clear"] > 0.15, "the inscribed radius leaves no bound"
    return out


def near_points(points, xy, bound, segs):
    """the distance of every xy to `points`, computed only where the walls themselves (on which the points lie) are within
    `bound`; inf elsewhere"""
    q = np.asarray(xy, np.float64).reshape(-1, 2)
    out = np.full(len(q), np.inf)
    close = st.dist_to(segs, q) <= bound
    out[close] = st.dist_to(points, q[close])
    return out.reshape(np.shape(xy)[:-1])


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
class Twins:
    """the numpy twins, fed the library's tables as every twin is"""

    def mounts(self, raws):
        rec, _ = ground.reference(raws, CAM, GP, gate_q16=api.ground_gate(CAM, GP, W, H), labels=False)
        return np.ascontiguousarray(rec["base_from_cam"], np.float32)

    def obstacles(self, raws, op, mounts):
        edges = api.beam_edges(op)
        if mounts is None:
            occ, _, _, ranges, _ = obstacles.reference(raws, CAM, op, edges)
            return occ, ranges
        outs = [obstacles.reference(r, CAM, dataclasses.replace(op, base_from_cam=tuple(float(v) for v in m)), edges) for r, m in zip(raws, mounts)]
        return np.stack([o[0] for o in outs]), np.stack([o[3] for o in outs])

    def costmap(self, cp, op, poses, occ, ranges):
        ref = costmap.Reference(cp, op, 1, api.beam_edges(op))
        q = api.costmap_pose_q(cp, op, poses)
        grid, logodds, _ = ref.push(q, occ, ranges)
        return grid, logodds, q

    def inflate(self, grid, ip):
        return inflate.reference(grid, ip, api.inflate_table(ip))[0]

    def navfn(self, cost, goals, starts, nav):
        return navfn.reference(cost, goals, starts, nav)

    def rollout(self, cost, pot, q5, rp, fp):
        return rollout.reference(cost, pot, q5, None, rp, *api.rollout_tables(rp, fp))


def world_cell(xy):
    return int(math.floor(xy[0] / CELL)), int(math.floor(xy[1] / CELL))


def run_chain(scene, be, mistake=None):
    """The whole chain for one scene on a backend -> a dict of everything it made.  `mistake` applies one of CAUGHT_BY's on this
    side of the chain: to what a stage is handed, never to a stage."""
    assert mistake is None or mistake in CAUGHT_BY, mistake
    poses = np.asarray(scene.poses, np.float64)
    raws = np.stack([st.render(scene, p) for p in poses])
    op, cp = OP, costmap_params(scene)
    mounts = be.mounts(raws) if scene.fitted_mount else None
    if mistake == "the mount's y taken as +X":
        flip = np.array([1, 1, 1, 1, -1, -1, -1, 1, 1, 1, 1, 1], np.float32)     # the row of y negated: y = +X
        op, mounts = dataclasses.replace(op, base_from_cam=tuple(float(v) for v in np.float32(LEVEL) * flip)), None if mounts is None else mounts * flip
    occ, ranges = be.obstacles(raws, op, mounts)
    R = dict(raws=raws, occ=occ, ranges=ranges, mounts=mounts)
    if mistake == "the obstacle grid flipped in y":
        occ = R["occ"] = np.ascontiguousarray(occ[:, ::-1])
    cm_poses, cm_op = poses, OP
    if mistake == "yaw negated for the costmap":
        cm_poses = poses * (1, 1, -1)
    if mistake == "gw and gh swapped":
        cm_op = dataclasses.replace(OP, gw=OP.gh, gh=OP.gw)
        occ = occ.reshape(-1, OP.gw, OP.gh)
    grid, logodds, q = be.costmap(cp, cm_op, cm_poses, occ, ranges)
    origin = (int(q[-1][4]), int(q[-1][5]))
    cost = be.inflate(grid[-1:], IP)
    pose = poses[-1]
    gx, gy = world_cell(scene.goal)
    sx, sy = world_cell(pose)
    goal = (gx, gy) if mistake == "the goal cell without the window origin" else (gx - origin[0], gy - origin[1])
    start = (sx - origin[0], sy - origin[1])
    pot, path, stats = be.navfn(cost, [goal], [start], NAV)[:3]
    ro_pose = pose * (1, 1, -1) if mistake == "yaw negated for the rollout" else pose
    ro_origin = (0.0, 0.0) if mistake == "the rollout's origin left at (0, 0)" else (origin[0] * CELL, origin[1] * CELL)
    q5 = api.rollout_pose_q(CELL, ro_origin[0], ro_origin[1], ro_pose[None])
    samples, best, traj = be.rollout(cost, pot, q5, RP, FOOTPRINT)
    R.update(grid=grid, logodds=logodds, q=np.asarray(q), origin=origin, cost=cost[0], pot=pot[0], path=path[0], nav_stats=stats[0], goal=goal,
             start=start, q5=q5, samples=samples[0], best=best[0], traj=traj[0], arc_sign=-1.0 if mistake == "the truth arc with -w" else 1.0)
    return R


# ---- the checks: each takes a scene's name and what the chain made, prints its chain_truth line and asserts ------------------------------
def grid_bounds(name, occupied, occupied_at, tag="chain_truth"):
    """Base frame, frame by frame.  An occupied cell's centre lies within sqrt(2)/2 c + dZ of a wall.  A cell that the truth gives
    at least min_obstacle_hits wall rays clear of every border (1e-3 c from a cell's edge and from the band's ends, plus E) is
    occupied: the rays that are clear fall in the cell whatever the others do.  That asks for every cell with min_obstacle_hits
    + 2 rays none of which is near a border, and for more.  The cells it leaves out are at most a fifth of those that received
    any ray.

    occupied[k]: the world xy (m, 2) of the centres of frame k's occupied cells; occupied_at(k, xy): whether the cell that holds
    each base-frame point xy (m, 2) of frame k is occupied."""
    T = truth(name)
    scene, worst, must_all, any_all, missing = T["scene"], 0.0, 0, 0, []
    edge = 1e-3 + T["fit"] / CELL
    for k, pose in enumerate(scene.poses):
        if len(occupied[k]):
            worst = max(worst, float(st.dist_to(T["segs"], occupied[k]).max()))
        _, idx, near, _ = st.wall_rays(scene, pose, GRID, (Z_BAND[0] - T["fit"], Z_BAND[1] + T["fit"]), edge)
        key = idx[:, 1] * GRID[3] + idx[:, 0]
        cells = np.unique(key)
        sure = np.array([np.count_nonzero(~near[key == c]) for c in cells])
        must = cells[sure >= MIN_HITS]
        any_all, must_all = any_all + len(cells), must_all + len(must)
        got = occupied_at(k, np.stack([GRID[0] + (must % GRID[3] + 0.5) * CELL, GRID[1] + (must // GRID[3] + 0.5) * CELL], -1))
        missing += [(k, int(c % GRID[3]), int(c // GRID[3])) for c in must[~np.asarray(got, bool)]]
    share = 1.0 - must_all / any_all
    bound = SQ2 / 2 * CELL + T["tol"]
    print(f"{tag} {name} | grid | occupied centre to wall {worst:.4f} m <= {bound:.4f} m | required cells {must_all} of {any_all}, left out {share:.3f} <= 0.2")
    assert worst <= bound, (worst, bound)
    assert share <= 0.2, share
    assert not missing, missing[:10]


def check_grid(name, R):
    """grid_bounds on the api's arrays: cell (ix, iy) of occ[k] covers [x_min + ix c, + c) x [y_min + iy c, + c) of the base frame"""
    occupied = []
    for k, pose in enumerate(truth(name)["scene"].poses):
        iy, ix = np.nonzero(R["occ"][k] == 100)
        occupied.append(st.to_world(pose, np.stack([GRID[0] + (ix + 0.5) * CELL, GRID[1] + (iy + 0.5) * CELL], -1)))

    def occupied_at(k, xy):
        ix, iy = np.floor((xy[:, 0] - GRID[0]) / CELL).astype(np.int64), np.floor((xy[:, 1] - GRID[1]) / CELL).astype(np.int64)
        return R["occ"][k][iy, ix] == 100
    grid_bounds(name, occupied, occupied_at)


def _first_hit(origin, angles, segs):
    """2-D: the distance from origin along every angle to the first vertical face, inf without one"""
    d = np.stack([np.cos(angles), np.sin(angles)], -1)
    out = np.full(len(angles), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for x0, y0, x1, y1, _ in segs:
            ex, ey = x1 - x0, y1 - y0
            den = d[:, 0] * ey - d[:, 1] * ex
            t = ((x0 - origin[0]) * ey - (y0 - origin[1]) * ex) / den
            s = ((x0 - origin[0]) * d[:, 1] - (y0 - origin[1]) * d[:, 0]) / den
            out = np.where((den != 0) & (t > 0) & (s >= 0) & (s <= 1) & (t < out), t, out)
    return out


def scan_bounds(name, ranges, sector, tag="chain_truth"):
    """Each finite range lies between the truth's nearest and farthest first wall along the beam, its two edges included, less
    and plus dZ: the form of test_obstacles.py's known answer, with the beam's inside sampled as well so that a wall's end or a
    box's corner inside a beam is allowed for.

    ranges[k][b]: frame k's range of beam b; sector(b) -> the two base-frame angles between which beam b looks."""
    T = truth(name)
    scene, worst, count = T["scene"], -np.inf, 0
    for k, pose in enumerate(scene.poses):
        for b in np.nonzero(np.isfinite(ranges[k]))[0]:
            lo, hi = sector(int(b))
            hits = _first_hit(pose[:2], pose[2] + lo + np.linspace(0.0, 1.0, 65) * (hi - lo), T["segs"])
            hits = hits[np.isfinite(hits)]
            assert hits.size, (k, b, "a return where the truth has no wall")
            r = float(ranges[k][b])
            over = max(hits.min() - r, r - hits.max())
            worst, count = max(worst, over), count + 1
    print(f"{tag} {name} | scan | {count} returns, furthest outside the truth's span {worst:.5f} m <= {T['tol']:.5f} m")
    assert count >= 10 * len(scene.poses) and worst <= T["tol"], (count, worst)


def check_scan(name, R):
    """scan_bounds on the api's ranges: beam b covers [angle_min + b * increment, + increment)"""
    a0, da = float(np.float32(OP.angle_min_rad)), float(np.float32(OP.angle_increment_rad))
    scan_bounds(name, R["ranges"], lambda b: (a0 + b * da, a0 + (b + 1) * da))


UNKNOWN, FREE, OCCUPIED = -1, 0, 1            # what costmap_bounds and scroll_bounds read a cell as


def costmap_bounds(name, centres, state, tag="chain_truth"):
    """World frame, after the whole clip (see the module's docstring for D).  No known-free cell lies more than 1.5 c (+ E)
    inside what is hidden from every pose of the clip while also more than sqrt(2) c from every wall: the shadow of a wall and
    the inside of a box stay unknown.

    centres (mh, mw, 2): the world xy of every cell's centre; state (mh, mw): UNKNOWN, FREE or OCCUPIED."""
    T = truth(name)
    scene = T["scene"]
    occupied = centres[state == OCCUPIED]
    assert len(occupied) >= 10, "nothing is occupied"
    far = float(st.dist_to(T["any_ray"], occupied).max())
    lone = float(st.dist_to(occupied, T["sure"]).max())
    free = state == FREE
    # "beyond by more than 1.5 c": nothing within 1.5 c of the centre (the centre, and two rings around it) is seen from any pose
    ring = np.array([(0.0, 0.0)] + [(r * math.cos(a), r * math.sin(a)) for r, m in ((0.75, 16), (1.5, 32)) for a in np.arange(m) * 2 * math.pi / m])
    spots = centres[free][:, None, :] + ring[None] * (1.5 * CELL + T["fit"]) / 1.5
    seen = np.zeros(spots.shape[:2], bool)
    for pose in scene.poses:
        seen |= st.visible(scene, pose, spots)
    hidden = np.zeros(state.shape, bool)
    hidden[free] = ~seen.any(1)
    hidden &= st.dist_to(T["segs"], centres) > SQ2 * CELL + T["fit"]
    print(f"{tag} {name} | costmap | {len(occupied)} occupied, furthest from a seen wall point {far:.4f} m, seen wall point furthest from one "
          f"{lone:.4f} m, both <= {T['D']:.4f} m | free cells {int(free.sum())}, hidden ones {int(hidden.sum())}")
    assert far <= T["D"], (far, T["D"])
    assert lone <= T["D"], (lone, T["D"])
    assert free.sum() >= 100 and not hidden.any(), centres[hidden][:5]


def logodds_state(L):
    """the api's log-odds as costmap_bounds reads them: occupied is L > 0, free is L < 0"""
    return np.where(L == costmap.UNKNOWN_L, UNKNOWN, np.where(L > 0, OCCUPIED, np.where(L < 0, FREE, 2))).astype(np.int8)


def check_costmap(name, R):
    """costmap_bounds on the api's log-odds, and: the window's origin is the cell of the pose less half the window"""
    T = truth(name)
    assert R["origin"] == T["origins"][-1], (R["origin"], T["origins"][-1])
    costmap_bounds(name, st.cell_centres(T["origins"][-1], CELL, *T["scene"].window), logodds_state(R["logodds"][-1]))


def scroll_bounds(name, known, tag="chain_truth"):
    """The clip that re-centres the window.  A cell of the final window that lay outside an earlier window is known only if it
    came into view (the image's horizontal field widened by 1.5 c) after it last came in: what scrolled out and back is unknown
    again, however well it was seen before.

    known (mh, mw): element [j][i] is the world cell (ox + i, oy + j) of the truth's final origin."""
    T = truth(name)
    scene = T["scene"]
    mw, mh = scene.window
    ox, oy = T["origins"][-1]
    centres = st.cell_centres((ox, oy), CELL, mw, mh)
    i, j = np.meshgrid(ox + np.arange(mw), oy + np.arange(mh))
    entered = np.zeros((mh, mw), np.int64)
    for k, (px, py) in enumerate(T["origins"]):
        outside = ~((i >= px) & (i < px + mw) & (j >= py) & (j < py + mh))
        entered[outside] = k + 1
    shift = np.abs(np.asarray(T["origins"]) - T["origins"][0]).max()
    assert shift > max(mw, mh) // 2, "the window does not re-centre by more than half its width"
    after, before = np.zeros((mh, mw), bool), np.zeros((mh, mw), bool)
    for k, pose in enumerate(scene.poses):
        view = st.in_view(pose, centres, slack=1.5 * CELL + T["fit"])
        after |= view & (k >= entered)
        before |= view & (k < entered) & st.visible(scene, pose, centres)
    back = before & ~after                      # seen once, scrolled out, back and not seen since
    print(f"{tag} {name} | scroll | the window moved by {shift} cells of {max(mw, mh)} | {int(back.sum())} cells seen, scrolled out and back: "
          f"{int((back & known).sum())} known | known cells never in view since they came in: {int((known & ~after).sum())}")
    assert back.sum() >= 50, "no cell scrolled out and back"
    assert not (known & ~after).any()


def check_scroll(name, R):
    scroll_bounds(name, R["logodds"][-1] != costmap.UNKNOWN_L)


def inflation_bounds(name, centres, open_, tag="chain_truth"):
    """A cell whose cost is below 253, or 255 (unknown: sn_inflate_grid puts 253 or 254 over an unknown cell within the inscribed
    radius), keeps the clearance from every seen wall point; a cell within the clearance of one is at 253 or 254.

    centres (mh, mw, 2): the world xy of every cell's centre; open_ (mh, mw): the cell is below 253 or unknown."""
    T = truth(name)
    d = near_points(T["sure"], centres, T["clear"], T["segs"])
    nearest = float(d[open_].min())
    inside = d <= T["clear"]
    print(f"{tag} {name} | inflation | nearest passable cell to a seen wall point {nearest:.4f} m > {T['clear']:.4f} m | {int(inside.sum())} cells within "
          f"that: {int((inside & open_).sum())} passable")
    assert inside.sum() >= 50
    assert nearest > T["clear"] and not (inside & open_).any()


def check_inflation(name, R):
    T = truth(name)
    inflation_bounds(name, st.cell_centres(T["origins"][-1], CELL, *T["scene"].window), (R["cost"] < 253) | (R["cost"] == 255))


def path_world(name, R):
    n = int(R["nav_stats"][2])
    assert R["nav_stats"][0] == 0 and 2 <= n <= NAV.max_path, R["nav_stats"].tolist()
    cells = R["path"][:n].astype(np.int64)
    return cells, (cells + truth(name)["origins"][-1] + 0.5) * CELL


def check_path(name, R):
    """The path starts in the robot's cell and ends in the goal's; its steps are 8-connected and no diagonal squeezes past a
    blocked cell; every cell keeps the clearance; it crosses no wall and crosses the true opening; its Euclidean length L lies
    between the zero-clearance geodesic and the witness's bound.

    The upper bound.  The witness keeps inflation radius + 2 c from every wall, so the cells within one cell of it cost 0 (or are
    unknown, priced at 0 as well), and each of its segments of length l has an 8-connected digitisation through such cells of at
    most one cell more than 1.0824 l / c straight-equivalent steps (1.0824 = the worst ratio of the octile to the Euclidean
    distance).  The field minimises the sum of (neutral + cost) * (5 | 7), so the path's sum is at most neutral * 5 * (1.0824 *
    L_witness / c + segments).  The path's own sum is at least neutral * (5 straight + 7 diagonal) >= neutral * 5 * (L / c) /
    1.0102, since 7 stands for 5 sqrt(2) = 7.0711.  So L <= 1.0824 * 1.0102 * L_witness + 1.0102 c per segment, and the
    assertion takes one cell per segment on top of the product, which the factor on the segments' term (1 %) does not move."""
    T = truth(name)
    scene = T["scene"]
    cells, xy = path_world(name, R)
    ox, oy = T["origins"][-1]
    sx, sy = world_cell(scene.poses[-1])
    gx, gy = world_cell(scene.goal)
    assert tuple(cells[0]) == (sx - ox, sy - oy), ("the path does not start in the robot's cell", cells[0], (sx - ox, sy - oy))
    assert tuple(cells[-1]) == (gx - ox, gy - oy), ("the path does not end in the goal's cell", cells[-1], (gx - ox, gy - oy))
    step = np.diff(cells, axis=0)
    assert np.all(np.abs(step).max(1) == 1), "a step that is not to a neighbour"
    blocked = (R["cost"] >= 253) & (R["cost"] != 255)
    assert not blocked[cells[:, 1], cells[:, 0]].any()
    diag = np.abs(step).sum(1) == 2
    assert not (blocked[cells[:-1, 1] + step[:, 1], cells[:-1, 0]] | blocked[cells[:-1, 1], cells[:-1, 0] + step[:, 0]])[diag].any(), "a cut corner"
    path_bounds(name, xy)


def path_bounds(name, xy, tag="chain_truth"):
    """the part of check_path that speaks of metres alone: xy (n, 2) are the world positions of the path's cells, start first"""
    T = truth(name)
    scene = T["scene"]
    clearance = float(near_points(T["sure"], xy, T["clear"] + 1.0, T["segs"]).min())
    assert not st.crosses_walls(scene, xy), "the path goes through a wall"
    gate = [st.crossing(a, b, *scene.gate) for a, b in zip(xy[:-1], xy[1:])]
    at = [a + t * (b - a) for a, b, t in zip(xy[:-1], xy[1:], gate) if t is not None]
    length = st.polyline_length(xy)
    lo = st.polyline_length(st.geodesic(scene))
    wit = st.witness(scene)
    assert st.witness_clearance(scene) >= INFLATION + 2 * CELL - 1e-9 and not st.crosses_walls(scene, st.geodesic(scene))
    hi = 1.0824 * 1.0102 * st.polyline_length(wit) + CELL * (len(wit) - 1)
    print(f"{tag} {name} | path | {len(xy)} cells, clearance {clearance:.4f} m > {T['clear']:.4f} m | crosses the opening at "
          f"{[tuple(round(float(v), 3) for v in p) for p in at]} | length {lo:.4f} <= {length:.4f} <= {hi:.4f} m")
    assert clearance > T["clear"]
    assert len(at) == 1, "the path does not cross the opening once"
    assert lo - 1e-9 <= length <= hi, (lo, length, hi)


def command(R):
    """(v, w) of the best sample by the lattice of the contract: v_min + iv * (v_max - v_min) / (nv - 1), w likewise"""
    assert R["best"][0] == 0, ("no valid sample", R["best"].tolist())
    iv, iw = divmod(int(R["best"][1]), RP.nw)
    return RP.v_min + iv * (RP.v_max - RP.v_min) / (RP.nv - 1), RP.w_min + iw * (RP.w_max - RP.w_min) / (RP.nw - 1)


def arc_bounds(name, v, w, xy, turns, arc_sign=1.0, tag="chain_truth"):
    """check_rollout's bound on the best sample's trajectory (derived there): the world positions xy (steps + 1, 2) lie within
    2 units of 1/256 cell per axis of the closed-form arc of (v, w) from the scene's last pose, and the headings `turns` (in
    turns, any branch) within 2 units of 1/65536 turn of the arc's -> the arc (x, y, heading)"""
    pose = np.asarray(truth(name)["scene"].poses[-1], np.float64)
    t = RP.sim_time_s * np.arange(RP.steps + 1) / RP.steps
    ax, ay, ah = st.arc(pose, v, arc_sign * w, t)
    assert np.shape(xy) == (RP.steps + 1, 2) and np.shape(turns) == (RP.steps + 1,), (np.shape(xy), np.shape(turns))
    off = float(np.abs(np.asarray(xy) - np.stack([ax, ay], -1)).max() / CELL * 256.0)
    turn = (np.asarray(turns) * 65536.0 - ah / (2 * math.pi) * 65536.0 + 32768.0) % 65536.0 - 32768.0
    print(f"{tag} {name} | rollout | command v {v:.3f} m/s w {w:+.2f} rad/s | traj off the arc by {off:.3f} <= 2 units of 1/256 cell, heading by "
          f"{float(np.abs(turn).max()):.3f} <= 2 units of 1/65536 turn")
    assert off <= 2.0 and np.abs(turn).max() <= 2.0, (off, float(np.abs(turn).max()))
    return ax, ay, ah


def check_rollout(name, R):
    """traj of the best sample against the closed-form arc, the footprint and the centre against the seen wall, the side the
    command turns to, and every sample the truth drives into a wall.

    The roundings of a trajectory point by the header's contract, per axis in units of 1/256 cell: the centre table's llrint
    (1/2), the pose's llrint (1/2), the rotation's + 2^29 >> 30 (1/2), and cq, sq rounded to 2^-30, which moves a centre at most
    2^21 units away by 2^-9: 1.502 in all, asserted as 2.  The heading, in 1/65536 turn: the table's llrint and the pose's, 1/2
    each: 1, asserted as 2.  Both are the figures the issue gives; the contract gives no more.

    A footprint point lies in a cell that is not occupied, and a centre in a cell below 253, so by the bounds of the map and of
    the inflation: no footprint point of the arc, placed by the truth, lies beyond a seen stretch of wall by more than sqrt(2) c
    + dZ (seen from the arc's centre at that step), and no centre within the clearance.  A sample whose centre, placed by the
    truth, comes within clearance - (sqrt(2)/2 + 2 sqrt(2)/256) c of a seen wall point at a step stands, as the kernel places it
    (2 units per axis off at most), in a cell whose centre is within the clearance: at 253 or 254, so the sample is not valid."""
    T = truth(name)
    scene = T["scene"]
    pose = np.asarray(scene.poses[-1], np.float64)
    v, w = command(R)
    t = RP.sim_time_s * np.arange(RP.steps + 1) / RP.steps
    origin = np.asarray(T["origins"][-1], np.float64)
    ax, ay, ah = arc_bounds(name, v, w, (origin + R["traj"][:, :2] / 256.0) * CELL, R["traj"][:, 2] / 65536.0, R["arc_sign"])
    centres = np.stack([ax, ay], -1)
    near = float(near_points(T["sure"], centres, T["clear"] + 1.0, T["segs"]).min())
    deepest, limit = 0.0, SQ2 * CELL + T["tol"]
    for k in range(RP.steps + 1):
        pts = st.to_world((ax[k], ay[k], ah[k]), FOOTPRINT.astype(np.float64))
        for p in pts:
            for s in T["segs"]:
                c = st.crossing(centres[k], p, s[0:2], s[2:4])
                if c is not None and st.dist_to(T["sure"], (centres[k] + c * (p - centres[k]))[None])[0] <= T["D"]:
                    deepest = max(deepest, float(st.dist_to(s[None], p[None])[0]))
    if scene.left:
        assert v > 0 and w * scene.left > 0, ("the command does not turn towards the way round", v, w)
    reasons = R["samples"][:, 1] >> 8 & 0xff
    inner = T["clear"] - (SQ2 / 2 + 2 * SQ2 / 256) * CELL
    driven = []
    for s in range(RP.nv * RP.nw):
        sv = RP.v_min + (s // RP.nw) * (RP.v_max - RP.v_min) / (RP.nv - 1)
        sw = RP.w_min + (s % RP.nw) * (RP.w_max - RP.w_min) / (RP.nw - 1)
        x, y, _ = st.arc(pose, sv, sw, t)
        if near_points(T["sure"], np.stack([x, y], -1), inner, T["segs"]).min() <= inner:
            driven.append(s)
    wrong = [s for s in driven if reasons[s] == rollout.VALID]
    print(f"chain_truth {name} | rollout | centre's clearance {near:.4f} m > {T['clear']:.4f} m, footprint beyond a seen wall by {deepest:.4f} m <= {limit:.4f} m | "
          f"{len(driven)} of {RP.nv * RP.nw} samples driven into a wall by the truth, {len(wrong)} of them valid | valid {int(R['best'][4])}")
    assert near > T["clear"] and deepest <= limit
    assert not wrong, wrong
    if scene.left:
        assert driven, "no sample reaches the wall"


CHECKS = {"grid": check_grid, "scan": check_scan, "costmap": check_costmap, "inflation": check_inflation, "path": check_path, "rollout": check_rollout}


def failures(name, R, checks=CHECKS):
    """the names of the checks that fail, with why"""
    out = {}
    for label, fn in checks.items():
        try:
            fn(name, R)
        except AssertionError as e:
            out[label] = str(e)[:200]
    return out


def mirror_bounds(a, A, B, cmd_a, cmd_b, tag="chain_truth"):
    """The mirrored world as a whole: each occupied cell of either final costmap has an occupied cell of the other, flipped in
    y, within one cell; the commands have the same v and opposite w within one step of the lattice.

    A, B (m, 2): the world cells (cx, cy) that are occupied in the scene's and in its mirror image's final costmap."""
    B = np.asarray(B) * (1, -1) - (0, 1)            # world cell cy covers [cy, cy + 1) c: its mirror image is cell -1 - cy
    gap = np.abs(np.asarray(A)[:, None, :] - B[None, :, :]).max(-1)
    (va, wa), (vb, wb) = cmd_a, cmd_b
    lattice = (RP.w_max - RP.w_min) / (RP.nw - 1)
    print(f"{tag} {a} | mirror | {len(A)} and {len(B)} occupied cells, furthest from its image {int(max(gap.min(1).max(), gap.min(0).max()))} <= 1 cell | "
          f"commands ({va:.3f}, {wa:+.2f}) and ({vb:.3f}, {wb:+.2f})")
    assert gap.min(1).max() <= 1 and gap.min(0).max() <= 1
    assert va == vb and abs(wa + wb) <= lattice + 1e-12, (va, wa, vb, wb)


def check_mirror(a, b, Ra, Rb):
    def cells(name, R):
        ox, oy = truth(name)["origins"][-1]
        j, i = np.nonzero(R["logodds"][-1] > 0)
        return np.stack([i + ox, j + oy], -1)
    mirror_bounds(a, cells(a, Ra), cells(b, Rb), command(Ra), command(Rb))


@functools.lru_cache(maxsize=None)
def twin_chain(name):
    """the twins' chain of a scene, computed once, shared and never changed"""
    R = run_chain(st.SCENES[name], Twins())
    for v in R.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return R


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
def test_the_scenes_are_what_they_claim():
    """what the checks rest on, from scene_truth alone: the witnesses keep their distance, the geodesics cross no wall, the
    mirrored image is the mirror image, and the depth relation gives back a fronto-parallel wall"""
    for name, scene in st.SCENES.items():
        assert st.witness_clearance(scene) >= INFLATION + 2 * CELL - 1e-9, name
        assert not st.crosses_walls(scene, st.witness(scene)) and not st.crosses_walls(scene, st.geodesic(scene)), name
        assert st.polyline_length(st.geodesic(scene)) <= st.polyline_length(st.witness(scene))
    for name in ("free end", "gap and box", "corridor", "free end pitched"):
        a, b = st.SCENES[name], st.SCENES[name + " mirrored"]
        for pa, pb in zip(a.poses, b.poses):
            assert np.array_equal(st.render(a, pa), st.render(b, pb)[:, ::-1]), name
    raw = st.render(st.FREE_END, (0.0, 0.0, 0.0))
    assert raw[5, 95] == raw[10, 60] == round(80.0 * 120.0 / (3.0 * 192000.0) / 2.60443857769133e-6)      # the wall at Z = 3 m
    assert raw[63, 50] == round(80.0 * 120.0 / (0.5 * 80.0 / 42.5 * 192000.0) / 2.60443857769133e-6)       # the ground under row 63
    x, y, h = st.arc((1.0, 2.0, math.pi / 2), 0.5, 1.0, math.pi)                                        # half a circle of radius 0.5 to the left
    assert abs(x - 0.0) < 1e-12 and abs(y - 2.0) < 1e-12 and abs(h - 1.5 * math.pi) < 1e-12
    x, y, h = st.arc((0.0, 0.0, 0.0), 1.0, 1e-12, 2.0)
    assert abs(x - 2.0) < 1e-9 and abs(y) < 1e-9


@pytest.mark.parametrize("name", list(st.SCENES))
def test_chain_against_the_truth(name):
    R = twin_chain(name)
    checks = dict(CHECKS, scroll=check_scroll) if st.SCENES[name].window != (100, 100) else CHECKS
    bad = failures(name, R, checks)
    assert not bad, bad


@pytest.mark.parametrize("name", ["free end", "gap and box", "corridor", "free end pitched"])
def test_the_mirrored_world(name):
    check_mirror(name, name + " mirrored", twin_chain(name), twin_chain(name + " mirrored"))


@pytest.mark.parametrize("mistake", list(CAUGHT_BY))
def test_every_mistake_is_caught(mistake):
    """the checks have teeth: each convention got wrong on this side of the chain fails the check that is there for it"""
    R = run_chain(st.FREE_END, Twins(), mistake)
    bad = failures("free end", R)
    print(f"chain_truth free end | mistake | {mistake}: caught by {sorted(bad)}")
    assert CAUGHT_BY[mistake] in bad, (mistake, bad)
