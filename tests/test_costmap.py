"""The rolling log-odds costmap (sn_costmap, hobot_stereonet_amd/costmap.py) without a GPU: the vectorised twin against the
plain loop over Python integers written from the header, the Python pose quantiser against sn_costmap_pose_q (pure host: a
costmap created without a handle serves it), the header's symbols and struct against the library and its ctypes mirror, the
parameter file, and the conditions that the inputs shared with tests/test_gpu_costmap.py must meet so that no comparison there
can pass vacuously: on them the twin alone takes every branch of the contract."""
import ctypes as C
import dataclasses
import math
import os
import re

import numpy as np
import pytest

from hobot_stereonet_amd import api, costmap
from hobot_stereonet_amd.costmap import CostmapParams
from hobot_stereonet_amd.obstacles import ObstacleParams

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_twin_equals_plain_loop_on_the_boundary_clip():
    p, op, poses, occ, ranges = costmap.boundary_clip()
    q = api.costmap_pose_q(p, op, poses)
    edges = api.beam_edges(op)
    twin, loop = costmap.Reference(p, op, edges=edges), costmap.LoopReference(p, op, edges=edges)
    assert _same(twin.push(q, occ, ranges), loop.push(q, occ, ranges))
    assert np.array_equal(twin.L[0], np.asarray(loop.L[0], np.int16))
    # one input absent, and a second push on the state the first left
    assert _same(twin.push(q[:3], occ[:3], None), loop.push(q[:3], occ[:3], None))
    assert _same(twin.push(q[3:], None, ranges[3:]), loop.push(q[3:], None, ranges[3:]))


@pytest.mark.parametrize("mw,mh,gw,gh,beams", [(7, 5, 5, 8, 1), (13, 9, 0, 0, 31), (1, 1, 5, 8, 8), (10, 11, 6, 4, 0)])
def test_twin_equals_plain_loop_on_random_clips_with_streams_and_reset(mw, mh, gw, gh, beams):
    p = CostmapParams(mw=mw, mh=mh, l_hit=90, l_miss=55, l_min=-130, l_max=170, clear_margin_m=0.05, clear_min_m=0.2, clear_max_m=0.0)
    op = ObstacleParams(x_min_m=-0.3, y_min_m=-0.45, cell_m=0.15, gw=gw, gh=gh, beams=beams, angle_min_rad=-1.1,
                        angle_increment_rad=2.2 / max(beams, 1))
    poses, occ, ranges = costmap.synthetic_clip(p, op, 9, seed=mw, step_m=0.2)
    q = np.array([costmap.pose_q(p, op, x) for x in poses])
    ids = [0, 1, 0, 2, 1, 0, 2, 2, 1]
    twin, loop = costmap.Reference(p, op, 3), costmap.LoopReference(p, op, 3)
    assert _same(twin.push(q[:5], occ[:5], ranges[:5], ids[:5]), loop.push(q[:5], occ[:5], ranges[:5], ids[:5]))
    twin.reset(1), loop.reset(1)
    assert _same(twin.push(q[5:], occ[5:], ranges[5:], ids[5:]), loop.push(q[5:], occ[5:], ranges[5:], ids[5:]))
    # a push of n maps equals n single pushes
    one = costmap.Reference(p, op, 3)
    parts = [one.push(q[k:k + 1], occ[k:k + 1], ranges[k:k + 1], ids[k:k + 1]) for k in range(5)]
    again = costmap.Reference(p, op, 3).push(q[:5], occ[:5], ranges[:5], ids[:5])
    assert _same([np.concatenate([part[i] for part in parts]) for i in range(3)], again)


def test_python_quantiser_is_within_one_unit_of_the_library():
    p, op = CostmapParams(mw=401, mh=77), ObstacleParams(cell_m=0.05)
    rng = np.random.default_rng(2)
    poses = np.concatenate([rng.uniform(-50, 50, (500, 3)), [[0, 0, 0], [0.0, 0.0, math.pi / 2], [-1e-9, 1e-9, math.pi], [200000.0, -200000.0, -7.5],
                                                             [0.025, -0.025, 1e-12]]])
    lib = api.costmap_pose_q(p, op, poses)
    py = np.array([costmap.pose_q(p, op, x) for x in poses])
    worst = int(np.abs(lib.astype(np.int64) - py).max())
    print(f"{len(poses)} poses: the two quantisers differ by at most {worst} unit")
    assert lib.dtype == np.int32 and worst <= 1
    assert np.array_equal(lib[:, [0, 1, 4, 5]], py[:, [0, 1, 4, 5]])      # the translation is one rounded product: the same bits
    assert lib[501].tolist()[2:4] == [0, 1 << 30]                         # yaw of exactly (double)pi/2: cq == 0
    k256 = 256.0 / float(np.float32(0.05))
    assert np.array_equal(lib[:, 4], (lib[:, 0] >> 8) - 200) and lib[504, 0] == round(0.025 * k256)
    # what the header refuses
    for bad in ([math.nan, 0, 0], [0, math.inf, 0], [0, 0, math.nan], [(2 ** 30 + 1) / k256, 0, 0], [0, -(2 ** 30 + 1) / k256, 0]):
        with pytest.raises(api.StereoNetError):
            api.costmap_pose_q(p, op, bad)
        with pytest.raises(ValueError):
            costmap.pose_q(p, op, bad)
    assert api.costmap_pose_q(p, op, [2 ** 30 / k256, 0, 0])[0] == 2 ** 30


def test_header_symbols_are_exported_and_the_struct_matches():
    lib = api.load_library()
    for sym in ("sn_costmap_create", "sn_costmap_reset", "sn_costmap_pose_q", "sn_costmap_push"):
        assert re.search(rf"\bint\s+{sym}\(", HEADER) and hasattr(lib, sym) and getattr(lib, sym).restype is C.c_int
    assert re.search(r"\bvoid sn_costmap_destroy\(", HEADER) and hasattr(lib, "sn_costmap_destroy")
    body = re.search(r"typedef struct sn_costmap_params \{(.*?)\} sn_costmap_params;", HEADER, re.S).group(1)
    fields = []
    for t, names in re.findall(r"^\s*(int|float)\s+([^;]+);", body, re.M):
        fields += [(nm.strip(), C.c_int if t == "int" else C.c_float) for nm in names.split(",")]
    assert fields == list(api.SnCostmapParams._fields_)
    assert [f for f, _ in fields] == [f.name for f in dataclasses.fields(CostmapParams) if f.name != "frame"]


def test_create_refuses_what_the_header_says_without_a_device():
    lib = api.load_library()
    good_p, good_op = CostmapParams(), ObstacleParams(beams=8, angle_min_rad=-0.5, angle_increment_rad=0.1)
    assert costmap.check(good_p, good_op) is None
    bad = [(dataclasses.replace(good_p, **kw), good_op) for kw in (
        dict(mw=0), dict(mh=4097), dict(l_hit=0), dict(l_miss=32768), dict(l_min=0), dict(l_min=-32768), dict(l_max=0), dict(l_max=32768),
        dict(clear_margin_m=-0.1), dict(clear_min_m=math.nan), dict(clear_max_m=math.inf))]
    bad += [(good_p, dataclasses.replace(good_op, **kw)) for kw in (
        dict(cell_m=0.0), dict(cell_m=math.nan), dict(x_min_m=math.inf), dict(gw=0), dict(gw=4097), dict(beams=-1), dict(beams=4097),
        dict(gw=0, gh=0, beams=0))]
    for p, op in bad:
        c = C.c_void_p()
        assert costmap.check(p, op) is not None, (p, op)
        assert lib.sn_costmap_create(None, 1, C.byref(api.obstacle_params(op)), C.byref(api.costmap_params(p)), C.byref(c)) == -1, (p, op)
        assert not c.value
    # a sector outside (-pi/2, pi/2): the beam table's refusal
    c = C.c_void_p()
    wide = dataclasses.replace(good_op, angle_increment_rad=0.5)
    assert lib.sn_costmap_create(None, 1, C.byref(api.obstacle_params(wide)), C.byref(api.costmap_params(good_p)), C.byref(c)) == -1
    # a costmap without a handle quantises poses and does nothing else
    assert lib.sn_costmap_create(None, 1, C.byref(api.obstacle_params(good_op)), C.byref(api.costmap_params(good_p)), C.byref(c)) == 0
    pose, grid = np.zeros(3), np.zeros(200 * 200, np.int8)
    occ = np.zeros(100 * 100, np.int8)
    assert lib.sn_costmap_push(c, 1, None, pose.ctypes.data, occ.ctypes.data, None, grid.ctypes.data, None, None, None, 0, None) == -1
    assert lib.sn_costmap_reset(c, 1) == -1 and lib.sn_costmap_reset(c, -1) == 0
    lib.sn_costmap_destroy(c)


def test_parameter_file_round_trip(tmp_path):
    p = CostmapParams(mw=123, mh=45, l_hit=7, l_miss=9, l_min=-11, l_max=13, clear_margin_m=0.1, clear_min_m=1 / 3, clear_max_m=7.25,
                      frame="map")
    path = str(tmp_path / "costmap.txt")
    costmap.save_params(path, p)
    assert costmap.load_params(path) == p
    with open(path, "a") as f:
        f.write("mw 3\n")
    with pytest.raises(ValueError):
        costmap.load_params(path)
    poses = tmp_path / "poses.txt"
    poses.write_text("# x y yaw\n0 0 0\n1.5 -2 0.25  # second\n")
    assert costmap.load_poses(str(poses)).tolist() == [[0, 0, 0], [1.5, -2, 0.25]]
    img = costmap.grid_image(np.array([[-1, 0, 100], [50, 0, 0]], np.int8))
    assert img.shape == (3, 2) and img[2, 1] == 128 and img[0, 1] == 0 and img[1, 1] == 255 and img[2, 0] == 127


def test_shared_inputs_take_every_branch():
    """The clip that tests/test_gpu_costmap.py compares on, through the twin alone with the library's q and beam table."""
    p, op, poses, occ, ranges = costmap.boundary_clip()
    q = api.costmap_pose_q(p, op, poses)
    twin = costmap.Reference(p, op, edges=api.beam_edges(op))
    grid, logodds, stats = twin.push(q, occ, ranges)
    fr = twin.frames
    total = {k: sum(f[k] for f in fr) for k in ("hit", "clear_occ", "clear_ray", "ray_edge", "ray_inside", "at_min", "at_max", "born")}
    print(total, [f["scrolled"] for f in fr])
    assert all(f["hit"] > 0 and f["clear_occ"] > 0 and f["clear_ray"] > 0 for f in fr)      # hits, clears through o == 0, through the ray only
    assert fr[0]["ray_edge"] == 1 and fr[0]["ray_inside"] == 1                               # r2 == C*C, and one sub inside
    u = costmap.units(p, op)
    assert q[0].tolist() == [128, 128, 1 << 30, 0, -12, -9] and u.margin == 128
    # ... which are the cells (4, 3) and (5, 0): not cleared (still unknown after three frames) and cleared (at the clamp)
    assert logodds[2, 3 + 9, 4 + 12] == costmap.UNKNOWN_L and logodds[2, 0 + 9, 5 + 12] == p.l_min
    assert total["at_min"] > 0 and total["at_max"] > 0 and (logodds == p.l_min).any() and (logodds == p.l_max).any()
    assert fr[0]["born"] > 0 and fr[3]["born"] > 0                                           # unknown -> known
    assert (grid == -1).any() and (grid == 0).any() and (grid == 100).any() and ((grid > 0) & (grid < 100)).any()
    # scrolls: by one cell, across the wrap column (the origin passes a multiple of mw), further than a window
    assert fr[3]["prev"] == (-12, -9) and fr[3]["origin"] == (-13, -9) and 0 < fr[3]["scrolled"] <= p.mh
    assert fr[5]["prev"][0] < 0 < fr[5]["origin"][0] and fr[5]["origin"][0] - fr[5]["prev"][0] < p.mw and fr[5]["scrolled"] > 0
    assert fr[6]["origin"][0] - fr[6]["prev"][0] > p.mw and fr[6]["scrolled"] == int(stats[5, 0]) > 0
    assert (q[:, 4:] < 0).any() and q[3, 0] < 0 and q[4, 1] < 0                              # negative world cells and translations
    assert q[4, 2] == 0 and q[5, 3] == 0 and q[5, 2] == -(1 << 30)                           # yaw of exactly pi/2 and pi
    # beams without a return clear nothing: with rays alone, the cells of the first three beams stay unknown
    only = costmap.Reference(p, op, edges=api.beam_edges(op))
    _, lo, st = only.push(q[:1], None, ranges[:1])
    assert st[0, 2] == 0 and 0 < st[0, 3] == st[0, 0] < p.mw * p.mh
    assert np.array_equal(stats[:, 0], (logodds != costmap.UNKNOWN_L).sum(axis=(1, 2)))
    assert np.array_equal(stats[:, 1], (logodds > 0).sum(axis=(1, 2)))
