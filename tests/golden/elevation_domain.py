"""The inputs the elevation map (sn_elevation_push) is judged on beside the constants of its launch: the geometries of
postproc_domain.GEOMETRIES at camera step 1, 2 and 4, a push of more maps than a launch takes (kSlice = 64) on three streams
with a mount per map, a launch whose row chunks the workgroup cap lengthens, a window of more cells than one pass of k_el_clear covers (2048 workgroups of 256), windows at the declared
limit of 4096 cells, and poses within a cell of the quantiser's limit.  tests/test_elevation_geometry.py checks on the CPU that
these inputs do what they are there for (points used, branches taken, the last column block carrying points, the mutated readings
of the slice walk differing); tests/test_gpu_elevation_geometry.py runs them on the MI355X against the twin, byte for byte.
Nothing here touches a GPU."""
import dataclasses
import functools

import numpy as np

import postproc_domain as dom
from hobot_stereonet_amd import elevation as el
from hobot_stereonet_amd import obstacles
from hobot_stereonet_amd.elevation import ElevationParams
from hobot_stereonet_amd.pointcloud import Camera

STEPS = (1, 2, 4)
N = 3
SLICE = 64                           # kSlice (csrc/sn_stream_groups.hpp)
CLEAR_PASS = 2048 * 256              # cells one pass of k_el_clear's grid covers
BASE = ElevationParams(mw=21, mh=18, cell_m=0.25, z_min_m=-1.0, z_max_m=1.5, range_max_m=8.0, min_points=1, alpha=96, max_step_mm=70,
                       radius=1)
CAM = Camera(fx=40.0, fy=40.0, baseline_mm=120.0)


GEOMETRIES, DEGENERATE, FULL, DMAX = dom.GEOMETRIES, dom.DEGENERATE, dom.FULL, dom.DMAX
# No geometry of the older stages' sweep is wider than 256 columns AND higher than 16 rows, so none gives k_el_scatter two column
# blocks of two row chunks each: blockIdx.x = cblock * chunks + chunk with both factors above 1.  One more geometry does.
EXTRA = {(300, 20): "two 256-column blocks x two row chunks of k_el_scatter at step 1 (Wo = 300, Ho = 20: chunks of 10 rows)"}
SWEEP = tuple(GEOMETRIES) + tuple(EXTRA)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- the geometry sweep ----------------------------------------------------------------------------------------------------------
# The recipe, adjusted where it does not give a full geometry's last map all three verdicts at every step.  A map much wider than
# high sees little ground under a focal length that follows its width: most of its points are the wall's, whose cells span more
# than 70 mm, so the threshold rises there until some of them are drivable; two geometries take another seed as well.
ADJUST = {(63, 15): dict(seed=7, max_step_mm=500), (64, 16): dict(seed=4, max_step_mm=500), (241, 17): dict(max_step_mm=300)}


@functools.lru_cache(maxsize=None)
def case(w, h, step):
    """-> (parameters, camera, poses (3, 3), maps int32 (3, h, w)) of the sweep at w x h: a 21 x 18 window of 0.25 m cells, the
    camera of tests/test_gpu_elevation.py's small maps (the focal length follows the width, the horizon is the first row of a map
    of fewer than four rows), a 3-frame clip of elevation.synthetic_clip.  A map of at most 16 pixels keeps every sample."""
    cam = dataclasses.replace(CAM, fx=0.4 * max(w, 2), fy=0.4 * max(w, 2), step=step, cx=w / 2.0, cy=0.0 if h < 4 else h / 2.0)
    adjust = ADJUST.get((w, h), {})
    p = dataclasses.replace(BASE, max_step_mm=adjust.get("max_step_mm", BASE.max_step_mm))
    poses, raw = el.synthetic_clip(p, w, h, cam, N, seed=adjust.get("seed", w + N))
    if w * h <= 16:
        raw[raw <= 0] = 900
    return (p, cam) + _frozen(poses, raw)


# ---- the slice walk: 130 maps on three streams, then 70 of them backwards after reset(1) -----------------------------------------
BIG, SECOND = 130, 70
WALK_W = WALK_H = 8
WALK = ElevationParams(mw=24, mh=18, cell_m=0.25, z_min_m=-1.0, z_max_m=1.5, range_max_m=8.0, min_points=1, alpha=96, max_step_mm=70,
                       radius=2)
WALK_CAM = dataclasses.replace(CAM, fx=0.4 * WALK_W, fy=0.4 * WALK_W, cx=WALK_W / 2.0, cy=WALK_H / 2.0)


def walk_ids():
    """the stream ids of tests/test_gpu_postproc_geometry.py's slice walks: 0 and 1 alternate in the first launch, all three take
    turns in the second (stream 2 is fresh there, alone), the third launch (2 maps) holds streams 2 and 0; then 70 maps in turn"""
    first = [k % 2 for k in range(SLICE)] + [k % 3 for k in range(SLICE, 2 * SLICE)] + [2, 0]
    assert len(first) == BIG and 2 not in first[:SLICE] and {0, 1, 2} == set(first[SLICE:2 * SLICE])
    return first, [k % 3 for k in range(SECOND)]


def launches(n):
    return [min(SLICE, n - k0) for k0 in range(0, n, SLICE)]


@functools.lru_cache(maxsize=None)
def walk():
    """-> (poses (130, 3), maps int32 (130, 8, 8), mounts float32 (130, 12)): a random walk of 0.6 cells a map (a stream moves by
    two or three of them between its frames) and a mount per map: height and pitch differ slightly by k"""
    poses, raw = el.synthetic_clip(WALK, WALK_W, WALK_H, WALK_CAM, BIG, seed=130, step_cells=0.6)
    mounts = np.asarray([obstacles.mount(0.0, 0.002 * (k % 7), (0.0, 0.0, 0.001 * k)) for k in range(BIG)], np.float32)
    return _frozen(poses, raw, mounts)


def walk_flow(push, reset):
    """The flow of the slice walk on any object with push(poses, maps, mounts, ids) and reset(stream): one push of 130,
    reset(1), then the first 70 maps with their poses reversed, the streams in turn."""
    poses, raw, mounts = walk()
    ids1, ids2 = walk_ids()
    push(poses, raw, mounts, ids1)
    reset(1)
    push(np.ascontiguousarray(poses[:SECOND][::-1]), raw[:SECOND], mounts[:SECOND], ids2)


def walk_q():
    poses, _, _ = walk()
    q = np.stack([el.pose_q(WALK, x) for x in poses])
    return q, np.ascontiguousarray(q[:SECOND][::-1])


# ---- a launch whose row chunks the workgroup cap shortens ------------------------------------------------------------------------
# sn_elevation_push gives k_el_scatter chunks of 16 rows until column blocks x chunks x maps passes about 2048 workgroups; from
# there on the chunks grow.  64 maps of one column block and 520 rows: 32 chunks by the cap against 33 of 16 rows, so 31 chunks of
# 17 rows, the last one of 10.
CAP_W, CAP_H, CAP_N = 3, 520, 64
CAP_CAM = dataclasses.replace(CAM, cx=CAP_W / 2.0, cy=CAP_H / 2.0)


def cap_chunks(ho=CAP_H, cblocks=1, m=CAP_N):
    """-> (chunks, rows) of the launch, by the launcher's rule"""
    chunks = max(1, min((2048 + cblocks * m - 1) // (cblocks * m), (ho + 15) // 16))
    rows = (ho + chunks - 1) // chunks
    return (ho + rows - 1) // rows, rows


@functools.lru_cache(maxsize=None)
def capped():
    """-> (poses (64, 3), maps (64, 520, 3)): a clip of one stream under the sweep's parameters"""
    return _frozen(*el.synthetic_clip(BASE, CAP_W, CAP_H, CAP_CAM, CAP_N, seed=64, step_cells=0.6))


# ---- more cells than one pass of k_el_clear --------------------------------------------------------------------------------------
BIG_WINDOW = ElevationParams(mw=700, mh=260, cell_m=0.02, z_min_m=-1.0, z_max_m=1.5, range_max_m=8.0, min_points=1, alpha=96,
                             max_step_mm=70, radius=3)
BIG_W, BIG_H = 96, 64


@functools.lru_cache(maxsize=None)
def big_window():
    """-> (poses (3, 3), maps (3, 64, 96)): 3 x 700 x 260 = 546 000 cells, more than the 524 288 the first pass of k_el_clear
    starts; the robot looks to its left front, so that the wall's and the ground's points lie around the cell CLEAR_PASS / 3"""
    _, raw = el.synthetic_clip(BIG_WINDOW, BIG_W, BIG_H, CAM, N, seed=7)
    poses = np.array([[0.0, 0.0, 0.85], [0.05, -0.3, 0.8], [0.02, -0.24, 0.9]])
    return _frozen(poses, raw)


# ---- windows at the declared limit -----------------------------------------------------------------------------------------------
LIMIT_CAM = dataclasses.replace(CAM, cx=48.0)      # column 48 looks straight ahead: y = 0 in the base frame


def limit_case(mw, mh):
    """-> (parameters, poses (2, 3), maps (2, 64, 96)) for a window of 4096 cells of 1 cm one way and 1 or 3 the other: it lies
    along the ground ahead of the robot (yaw 0 for a window long in x, a quarter turn for one long in y), the robot stands in the
    middle of a cell, and the second frame is 16 m further back along the window, so that the farthest cells of the first leave
    it.  radius 3: the verdict's halo is wider than the window."""
    p = ElevationParams(mw=mw, mh=mh, cell_m=0.01, z_min_m=-1.0, z_max_m=1.5, range_max_m=8.0, min_points=1, alpha=96, max_step_mm=70, radius=3)
    raw = np.stack([el.terrain_map(BIG_W, BIG_H, LIMIT_CAM, 0.4, 6.0, seed=40 + k, rough_m=0.01, holes=0.05) for k in range(2)])
    along_x = mw >= mh
    yaw = 0.0 if along_x else np.pi / 2
    poses = np.array([[0.005, 0.005, yaw], [-15.995, 0.005, yaw] if along_x else [0.005, -15.995, yaw]])
    return (p,) + _frozen(poses, raw)


LIMITS = ((4096, 1), (1, 4096), (4096, 3))


# ---- poses at the far limit ------------------------------------------------------------------------------------------------------
FAR = ElevationParams(mw=70, mh=33, cell_m=0.25, z_min_m=-1.0, z_max_m=1.5, range_max_m=8.0, min_points=1, alpha=96, max_step_mm=70, radius=2)


@functools.lru_cache(maxsize=None)
def far_poses():
    """-> (poses (4, 3), maps (4, 64, 96), stream ids): two streams, one in the corner (+, -) and one in the corner (-, +) of the
    quantiser's domain |x * 256 / cell_m| <= 2^30, looking nearly backwards (yaw near +pi and -pi).  Each starts on the limit itself
    and then steps back by one cell, across the last cell boundary, so its window scrolls there."""
    lim = 2.0 ** 30 / el.units(FAR).k256
    c = float(np.float32(FAR.cell_m))
    _, raw = el.synthetic_clip(FAR, BIG_W, BIG_H, CAM, 4, seed=17)
    poses = np.array([[lim, -lim, 3.1], [lim - c, -lim + c, 3.0], [-lim, lim, -3.1], [-lim + c, lim - c, -3.0]])
    return _frozen(poses, raw) + ([0, 0, 1, 1],)


